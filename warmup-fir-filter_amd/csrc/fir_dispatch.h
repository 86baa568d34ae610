// fir_dispatch.h — host only: the steps from a run-time argument to a template argument, each
// written once.  A visitor is a generic lambda that receives tag VALUES (TypeTag<T>{} for a
// sample type, IntTag<V>{} for an integer) and names the instantiation it wants from them:
//
//     with_io(in_dtype, stage, [&](auto t, auto st) {
//         return launch_x<typename decltype(t)::type, st>(args...);   // st converts to its int
//     });
//
// The arguments are the launchers' checked ones (check_fir1d and the others in fir_launch.h): an
// in_dtype that is not FIR_IN_U8 is FIR_IN_I16, a stage that is not FIR_OUT_U8_SAT is FIR_OUT_I32.
// Every visitor is instantiated for EVERY tag combination its helper can pass, so a helper must
// pass exactly the combinations that exist (with_reg_config).
#pragma once

#include <stdint.h>

#include <type_traits>

#include "fir_hip.h"

namespace fir {

template <typename T>
struct TypeTag {
    using type = T;
};
template <int V>
using IntTag = std::integral_constant<int, V>;

// f(IntTag<STAGE>{}): the output stage
template <typename F>
auto with_stage(int stage, F&& f) {
    return stage == FIR_OUT_U8_SAT ? f(IntTag<FIR_OUT_U8_SAT>{}) : f(IntTag<FIR_OUT_I32>{});
}

// f(TypeTag<InT>{}, IntTag<STAGE>{}): sample type x output stage
template <typename F>
auto with_io(int in_dtype, int stage, F&& f) {
    return in_dtype == FIR_IN_U8 ? with_stage(stage, [&](auto st) { return f(TypeTag<uint8_t>{}, st); })
                                 : with_stage(stage, [&](auto st) { return f(TypeTag<int16_t>{}, st); });
}

// f(TypeTag<InT>{}, IntTag<STAGE>{}, IntTag<CH>{}): the six single-filter configurations of the
// register kernel that fir1d_reg_inst.hip is compiled for (INSTS in the Makefile): u8 samples of
// one channel, int16 samples of one or two (reg_path_ok admits no other).  uint8_t with two
// channels is deliberately absent: no object defines that launcher, and the library links with
// undefined symbols allowed.
template <typename F>
auto with_reg_config(int in_dtype, int stage, int ch, F&& f) {
    return with_stage(stage, [&](auto st) {
        if (in_dtype == FIR_IN_U8) return f(TypeTag<uint8_t>{}, st, IntTag<1>{});
        if (ch == 1) return f(TypeTag<int16_t>{}, st, IntTag<1>{});
        return f(TypeTag<int16_t>{}, st, IntTag<2>{});
    });
}

// f(IntTag<v>{}) for v in [Lo, Hi], `invalid` outside it: a tap or filter count as a template
// argument.
template <int Lo, int Hi, typename R, typename F>
R with_int(int v, R invalid, F&& f) {
    if constexpr (Lo > Hi) {
        return invalid;
    } else {
        return v == Lo ? f(IntTag<Lo>{}) : with_int<Lo + 1, Hi>(v, invalid, f);
    }
}

}  // namespace fir
