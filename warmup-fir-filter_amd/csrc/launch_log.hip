// launch_log.hip — the launch record behind FIR_LAUNCH (fir_launch.h): the census of every kernel
// instantiation a launch site names, and the per-thread log of the launches a thread made while
// it had the log on.  Host code only; no launch is made here, and nothing is resolved to a name
// until a record is read.
#include <cxxabi.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "fir1d_reg.h"
#include "fir2d_reg.h"
#include "fir_launch.h"

namespace fir {

thread_local bool t_launch_log_on = false;

namespace {

constexpr size_t kLogMax = 4096;  // launches kept per thread

struct LaunchRec {
    const void* kernel;
    unsigned grid[3], block[3];
    std::string note;
};

struct ThreadLog {
    std::vector<LaunchRec> recs;
    size_t dropped = 0;
    bool begun = false;  // _begin seen and the log not yet read
};
thread_local ThreadLog t_log;

// Function-local statics: Site<K>::reg's initialisers run in no fixed order against this file's.
std::mutex& census_mu() {
    static std::mutex mu;
    return mu;
}
std::set<const void*>& census() {
    static std::set<const void*> s;
    return s;
}

// Template arguments of a demangled kernel name, split at depth-0 commas of its first <...>.
std::vector<std::string> template_args(const std::string& name) {
    std::vector<std::string> out;
    const size_t paren = name.find('(');
    const size_t lt = name.find('<');
    if (lt == std::string::npos || (paren != std::string::npos && lt > paren)) return out;
    int depth = 0;
    std::string cur;
    for (size_t i = lt; i < name.size(); ++i) {
        const char c = name[i];
        if (c == '<' || c == '(' || c == '[') {
            if (depth++ > 0) cur += c;
        } else if (c == '>' || c == ')' || c == ']') {
            if (--depth == 0) break;
            cur += c;
        } else if (c == ',' && depth == 1) {
            out.push_back(cur);
            cur.clear();
        } else if (!(c == ' ' && cur.empty())) {
            cur += c;
        }
    }
    if (!cur.empty()) out.push_back(cur);
    return out;
}

template <size_t N>
std::string spell(int v, const FlagName (&names)[N]) {
    std::string s;
    for (const FlagName& f : names)
        if ((v & f.mask) == f.value) s += (s.empty() ? "" : "|") + std::string(f.name);
    return s;
}

// The kernels whose template arguments hold a bit mask: which argument, and its names.
std::string flags_of(const std::string& name) {
    struct Masked {
        const char* kernel;
        size_t arg;
        bool mode2d;
    };
    static const Masked kMaskedKernels[] = {
        {"fir::fir1d_reg_kernel<", 5, false},
        {"fir::fir1d_reg_batch_kernel<", 5, false},
        {"fir::fir2d_reg_kernel<", 5, true},
        {"fir::fir2d_pk16_strip_kernel<", 3, true},
    };
    for (const Masked& m : kMaskedKernels) {
        if (name.find(m.kernel) == std::string::npos) continue;
        const std::vector<std::string> a = template_args(name);
        if (a.size() <= m.arg) return "?";
        char* end = nullptr;
        // an enum-typed argument demangles as "(fir::RegFlags)4162"
        const std::string& t = a[m.arg];
        const size_t close = t.rfind(')');
        const char* digits = t.c_str() + (close == std::string::npos ? 0 : close + 1);
        const long v = std::strtol(digits, &end, 10);
        if (end == digits) return "?";
        return m.mode2d ? spell((int)v, kMode2dNames) : spell((int)v, kRegFlagNames);
    }
    return "";
}

std::string kernel_name(const void* k) {
    const char* mangled = hipKernelNameRefByPtr(k, nullptr);
    if (!mangled) return "?";
    int status = 0;
    char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
    std::string s = status == 0 && d ? d : mangled;
    std::free(d);
    if (status != 0) {
        // a C++ runtime that does not know _Float16's code DF16_ yet: demangle with __fp16's (Dh,
        // a builtin type like it, so no substitution index moves) and put the name back
        std::string m = mangled;
        for (size_t i; (i = m.find("DF16_")) != std::string::npos;) m.replace(i, 5, "Dh");
        d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &status);
        if (status == 0 && d) {
            s = d;
            for (const char* half : {"__fp16", "half"})
                for (size_t i; (i = s.find(half)) != std::string::npos;) s.replace(i, std::strlen(half), "_Float16");
        }
        std::free(d);
    }
    return s;
}

std::string dims(const unsigned v[3]) {
    return std::to_string(v[0]) + "," + std::to_string(v[1]) + "," + std::to_string(v[2]);
}

int give(const std::string& text, char* buf, size_t cap, size_t* need, std::string* err) {
    if (!need) return *err = "need must not be NULL", FIR_EINVAL;
    *need = text.size() + 1;
    if (!buf || cap < *need)
        return *err = "buffer too small: " + std::to_string(*need) + " bytes needed", FIR_EINVAL;
    std::memcpy(buf, text.c_str(), *need);
    return FIR_OK;
}

}  // namespace

bool census_add(const void* kernel) {
    std::lock_guard<std::mutex> lk(census_mu());
    census().insert(kernel);
    return true;
}

void launch_log_add(const void* kernel, dim3 grid, dim3 block, const std::string& note) {
    ThreadLog& l = t_log;
    if (l.recs.size() >= kLogMax) {
        ++l.dropped;
        return;
    }
    l.recs.push_back({kernel, {grid.x, grid.y, grid.z}, {block.x, block.y, block.z}, note});
}

void launch_log_begin() {
    t_log.recs.clear();
    t_log.dropped = 0;
    t_log.begun = true;
    t_launch_log_on = true;
}

int launch_log_end(char* buf, size_t cap, size_t* need, std::string* err) {
    ThreadLog& l = t_log;
    t_launch_log_on = false;  // stops here; a too-small buffer keeps what was recorded for a retry
    if (need) *need = 0;
    if (!l.begun) return *err = "fir_launch_log_end without fir_launch_log_begin on this thread", FIR_EINVAL;
    if (l.dropped) {
        *err = "launch log overflow: " + std::to_string(l.dropped) + " launches past the first " +
               std::to_string(kLogMax) + " were dropped";
        l = ThreadLog();
        return FIR_EINVAL;
    }
    std::string text;
    for (const LaunchRec& r : l.recs) {
        const std::string name = kernel_name(r.kernel);
        text += name + "\t" + dims(r.grid) + "\t" + dims(r.block) + "\t" + flags_of(name) + "\t" + r.note + "\n";
    }
    const int rc = give(text, buf, cap, need, err);
    if (rc == FIR_OK) l = ThreadLog();
    return rc;
}

int kernel_census(char* buf, size_t cap, size_t* need, std::string* err) {
    std::vector<const void*> ks;
    {
        std::lock_guard<std::mutex> lk(census_mu());
        ks.assign(census().begin(), census().end());
    }
    std::vector<std::string> lines;
    for (const void* k : ks) {
        const std::string name = kernel_name(k);
        lines.push_back(name + "\t\t\t" + flags_of(name) + "\t\n");
    }
    std::sort(lines.begin(), lines.end());
    std::string text;
    for (const std::string& s : lines) text += s;
    return give(text, buf, cap, need, err);
}

}  // namespace fir
