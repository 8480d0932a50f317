"""Both gradients of the small nature CNN's second layer, Conv2d(16 -> 32, k 4, s 2) at 20 x 20 (csrc/conv_small.hip), against
aten.convolution_backward with the same operands in the same process, in alternating windows on one GPU: dx alone, dw alone
and both together (what fused._CONV2S_MIN_FRAMES is set from), with the achieved share of 8 TB/s at each frame count.  Both
sides are first held to the library's result in chunks of 2048 frames summed in float64.

    python tools/conv2s_probe.py [--frames 128,256,1024,4096,41472] [--out conv2s_probe.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rltime_amd.models.torch import fused                                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", default="128,256,1024,4096,41472")
ap.add_argument("--out", default="conv2s_probe.json")
args = ap.parse_args()
WINDOWS = 7
C, F, K, S, H, W = 16, 32, 4, 2, 20, 20
OH, OW = (H - K) // S + 1, (W - K) // S + 1
out = {}


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(name, new, old, reps, bytes_new):
    for _ in range(3):
        new(); old()                                                        # noqa: E702
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(WINDOWS):
        tn.append(window(new, reps))
        to.append(window(old, reps))
    rec = {"new_ms": [statistics.median(tn), min(tn), max(tn)], "library_ms": [statistics.median(to), min(to), max(to)],
           "new_wins_every_window": all(a <= b for a, b in zip(tn, to)),
           "new_share_of_8TBps": bytes_new / (statistics.median(tn) * 1e-3) / 8e12}
    out[name] = rec
    print(name, json.dumps(rec), flush=True)


def lib_bwd(g, x, wt, mask):
    return torch.ops.aten.convolution_backward(g, x, wt, None, [S, S], [0, 0], [1, 1], False, [0, 0], 1, mask)


for n in [int(v) for v in args.frames.split(",") if v]:
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(n, C, H, W, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    g = (torch.randn(n, F, OH, OW, device="cuda", generator=gen) * (torch.rand(n, F, OH, OW, device="cuda", generator=gen) < 0.5)) \
        .contiguous(memory_format=torch.channels_last)
    wt = torch.randn(F, C, K, K, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    assert fused.conv2s_supported(x, wt, (S, S), g, min_frames=0)
    dx, dw = fused.conv2s_bwd_data(g, wt, x), fused.conv2s_wgrad(g, x, wt)
    ref_dw = 0
    e_dx = 0.0
    for i in range(0, n, 2048):
        cdx, cdw, _ = lib_bwd(g[i:i + 2048], x[i:i + 2048], wt, [True, True, False])
        ref_dw = ref_dw + cdw.double()
        e_dx = max(e_dx, float((dx[i:i + 2048] - cdx).abs().max()))
    e_dw = float((dw.double() - ref_dw).abs().max())
    print("N=%d check: dx %.3e of %.3e, dw %.3e of %.3e" % (n, e_dx, float(dx.abs().max()), e_dw, float(ref_dw.abs().max())), flush=True)
    assert e_dx <= 1e-4 * float(dx.abs().max()) and e_dw <= 1e-4 * float(ref_dw.abs().max())
    b_g, b_x = 4.0 * n * OH * OW * F, 4.0 * n * H * W * C                  # g read + dx written; x and g read once
    reps = max(4, min(200, 400000 // n))
    tag = "N=%d " % n
    compare(tag + "dx", lambda: fused.conv2s_bwd_data(g, wt, x), lambda: lib_bwd(g, x, wt, [True, False, False]), reps, b_g + b_x)
    compare(tag + "dw", lambda: fused.conv2s_wgrad(g, x, wt), lambda: lib_bwd(g, x, wt, [False, True, False]), reps, b_g + b_x)
    compare(tag + "both", lambda: (fused.conv2s_bwd_data(g, wt, x), fused.conv2s_wgrad(g, x, wt)),
            lambda: lib_bwd(g, x, wt, [True, True, False]), reps, 2 * (b_g + b_x))
    del x, g, dx, dw
    torch.cuda.empty_cache()
json.dump(out, open(args.out, "w"), indent=1)
