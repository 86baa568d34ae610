"""Time fir_restore_u8_dev (normalize, and clip as the control) over 2^28 float64 samples.

    python tools/restore_rate.py LABEL [TREE]

TREE is a checkout (default: this one) holding warmup-fir-filter_amd/ with its built library, so
two versions of the library are compared by running this once per tree, alternating, in one
session.  HIP events around windows of 60 calls after 60 warm-up calls, 6 windows per policy, on a
seeded device-resident input; prints one JSON line (microseconds per call of every window, and a
checksum of the output so that two trees can be seen to compute the same bytes).
profiles/nonfinite/ holds the runs.
"""
import json
import sys
from pathlib import Path

label = sys.argv[1]
tree = str(Path(sys.argv[2] if len(sys.argv) > 2 else Path(__file__).resolve().parents[1]).resolve())
sys.path.insert(0, tree + "/warmup-fir-filter_amd")
import torch  # noqa: E402

import fir_hip  # noqa: E402
from fir_hip import torch_ops  # noqa: E402

assert fir_hip.lib_path().as_posix().startswith(tree), fir_hip.lib_path()
dev = torch.device("cuda:0")
n = 1 << 28
g = torch.Generator(device=dev)
g.manual_seed(5)
a = torch.empty(n, dtype=torch.float64, device=dev).uniform_(-300.0, 600.0, generator=g)
out = torch.empty(n, dtype=torch.uint8, device=dev)
work = torch.empty(int(fir_hip.lib().fir_restore_work_bytes()), dtype=torch.uint8, device=dev)
res = {"label": label, "n": n}
for name, policy in (("normalize", fir_hip.RESTORE_NORMALIZE), ("clip", fir_hip.RESTORE_CLIP)):
    for _ in range(60):
        torch_ops.restore_u8_dev(a, policy, out=out, work=work)
    torch.cuda.synchronize()
    wins = []
    for w in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(60):
            torch_ops.restore_u8_dev(a, policy, out=out, work=work)
        e1.record()
        torch.cuda.synchronize()
        wins.append(round(e0.elapsed_time(e1) * 1000.0 / 60, 2))
    res[name + "_us_per_call"] = wins
    res[name + "_checksum"] = int(out[::4099].to(torch.int64).sum().item())
print(json.dumps(res))
