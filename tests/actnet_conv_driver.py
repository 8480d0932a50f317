"""The conv comparisons of tests/test_actnet_exact_gpu.py, and, run as a program, the subprocess body of its RT = 2 test:
mirl_act_conv_fwd reads MIRL_ACT_CONV_WLDS once per process, so k_act_conv<.., RT = 2> (M > 8192 with the LDS-weights kernel
switched off) needs a process of its own.  As a program it runs layer 2 at 102 frames of 20x20 (M = 102 * 81 = 8262 = 258
workgroups of 32 rows + 6: the last workgroup's second 16-row tile is clamped throughout) and layer 3 at 169 frames of 9x9
(M = 169 * 49 = 8281), dyadic (bit-equal) and real (operation-count bound), prints one line per comparison and exits non-zero
on a mismatch."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import pointwise_restate as R          # noqa: E402

U = 2.0 ** -24
RT2_SHAPES = [(2, 102, 20, 20), (3, 169, 9, 9)]


def _p(t):
    return C.c_void_p(t.data_ptr())


def run_conv(layer, x, w, b):
    """x (F, Hi, Wi, C), w (64, C, k, k), b (64,) float64 -> the kernel's (F, Ho * Wo * 64) output on the CPU.  y is NaN-filled,
    64 floats wider than a frame's pixels, with a guard frame on either side: all of that must still be NaN."""
    from rltime_amd._lib import lib, check
    F_, Hi, Wi, ci = x.shape
    k, s = (4, 2) if layer == 2 else (3, 1)
    Ho, Wo = (Hi - k) // s + 1, (Wi - k) // s + 1
    n = Ho * Wo * 64
    pitch = n + 64
    y = torch.full((F_ + 2, pitch), float("nan"), device="cuda")
    xd = x.float().cuda().contiguous()
    wd = w.permute(0, 2, 3, 1).reshape(64, -1).float().cuda().contiguous()
    bd = b.float().cuda()
    assert lib.mirl_act_conv_supported(layer, ci, 64, k, s, Hi, Wi) == 1
    check(lib.mirl_act_conv_fwd(layer, F_, Hi, Wi, _p(xd), _p(wd), _p(bd), C.c_void_p(y.data_ptr() + 4 * pitch), pitch,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mirl_act_conv_fwd")
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isnan(y[F_ + 1]).all()), "a guard frame was written"
    assert bool(torch.isnan(y[1:F_ + 1, n:]).all()), "the padding of a frame's pitch was written"
    return y[1:F_ + 1, :n]


def dyadic_mismatches(layer, frames, Hi, Wi, seed):
    """-> (elements that differ from float64 relu(conv2d) or are -0 where it is 0, zeros planted, negatives planted)."""
    d = R.dyadic_conv(seed, layer, frames, Hi, Wi)
    assert d["margin"] < 2 ** 24
    pre = R.conv_relu_nhwc(d["x"], d["w"], d["b"], d["k"], d["s"], pre=True).reshape(frames, -1)
    want = torch.clamp(pre, min=0)
    got = run_conv(layer, d["x"], d["w"], d["b"])
    bad = int((got != want.float()).sum()) + int(torch.isnan(got).sum()) + int(torch.signbit(got[pre <= 0]).sum())
    if not torch.equal(got, want.float()):
        bad = max(bad, 1)
    return bad, int((pre == 0).sum()), int((pre < 0).sum()), pre.numel()


def real_ratio(layer, frames, Hi, Wi, seed):
    """rand / randn operands: worst |y - float64| / ((K + 1) u (sum |x w| + |b|)).  One accumulator per output takes all K
    products (16 K-steps of four 16x16x4 MFMAs at K = 512, 18 at K = 576, in every variant: k_act_conv RT = 1 and 2,
    k_act_conv_wlds), then the bias."""
    ci, k, s = (32, 4, 2) if layer == 2 else (64, 3, 1)
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(frames, Hi, Wi, ci, generator=g) * 2 - 0.5).double()
    w = (torch.randn(64, ci, k, k, generator=g) * 0.05).double()
    b = (torch.randn(64, generator=g) * 0.1).double()
    want = R.conv_relu_nhwc(x, w, b, k, s).reshape(frames, -1)
    mag = R.conv_relu_nhwc(x.abs(), w.abs(), b.abs(), k, s, pre=True).reshape(frames, -1)
    bound = (k * k * ci + 1) * U * mag
    err = (run_conv(layer, x, w, b).double() - want).abs()
    assert not bool(torch.isnan(err).any())
    return float((err / bound).max())


def main():
    assert os.environ.get("MIRL_ACT_CONV_WLDS") == "0"
    rc = 0
    for layer, frames, Hi, Wi in RT2_SHAPES:
        bad, zeros, neg, n = dyadic_mismatches(layer, frames, Hi, Wi, 4100 + layer)
        ratio = real_ratio(layer, frames, Hi, Wi, 4200 + layer)
        print("RT2 layer %d frames %d: %d of %d differ, %d exact zeros, %d negative" % (layer, frames, bad, n, zeros, neg))
        print("RATIO k_act_conv<RT=2> layer %d real: worst err / bound = %.3f" % (layer, ratio))
        if bad or not zeros or not neg or not ratio <= 1.0:
            rc = 1
    sys.stdout.flush()
    return rc


if __name__ == "__main__":
    sys.exit(main())
