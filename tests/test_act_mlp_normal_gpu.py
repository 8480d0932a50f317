"""GPU: csrc/act_mlp.hip k_act_mlp<true, true> (mirl_act_mlp_normal_fwd) — trunk, in-kernel standard-normal draws and Normal
head in one launch — through the C-ABI: the product row against mirl_act_mlp_ac_fwd's and the head against
mirl_actor_head_normal's, bit for bit; the draws against the float64 restatement of the keyed Philox block and Box-Muller."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import act_mlp_ac_restate as A
from tests import act_mlp_normal_restate as N

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", ["shipped", "no-leading-odd-D", "limits"])
def test_row_draws_and_head(name):
    from rltime_amd._lib import lib, check, ptr, stream
    case = N.Case(name)
    assert lib.mirl_act_mlp_normal_supported(*case.ac_shape_args()) == 1
    E, D, dc, logstd = case.E, case.D, A.DeviceCase(case), case.logstd.cuda()
    runs = [N.launch(dc, logstd, step) for step in N.STEPS]
    # the product row is mirl_act_mlp_ac_fwd's on the same operands with A = D: the same code
    logits = dc.launch(seed=N.RNG_SEED, step=N.STEPS[0])[2]
    assert bool(torch.isfinite(logits).all()) and torch.equal(_bits(runs[0][2]), _bits(logits))
    for step, (actions, policy, raw, eps) in zip(N.STEPS, runs):
        # both sides round ONE float64 value to float32 and the libm difference sits far below a float32 ulp: equal or neighbours
        want, dropped = N.draws(N.RNG_SEED, step, E, D)
        got = eps.cpu().numpy().astype(np.float64)
        bound = 2.0 ** -23 * np.maximum(np.abs(want), 2.0 ** -23)
        print("FIGURE", name, step, "max |eps - f64| / bound %.3f, max |eps| %.3f" % ((np.abs(got - want) / bound).max(), np.abs(got).max()))
        assert (np.abs(got - want) <= bound).all() and np.abs(got).max() <= 5.78
        assert D % 2 == 0 or (np.abs(got - dropped[:, None]) > 1e-6).all()      # no component holds the sine an odd D drops
        # actions, log-probability and value are mirl_actor_head_normal's on the row's means and value and these draws
        want_a, want_p, values = torch.full_like(actions, float("nan")), torch.full_like(policy, float("nan")), raw[:, D].contiguous()
        check(lib.mirl_actor_head_normal(E, D, ptr(raw), D + 1, ptr(logstd), ptr(values), ptr(eps), ptr(want_a),
                                         ptr(want_p), C.c_void_p(want_p.data_ptr() + 4), 2, stream()), "mirl_actor_head_normal")
        assert bool(torch.isfinite(actions).all()) and torch.equal(_bits(actions), _bits(want_a)) and torch.equal(_bits(policy), _bits(want_p))
    # a rerun on the same step word repeats to the bit; the next word changes every draw and nothing else; no draw is shared
    for x, y in zip(runs[0], N.launch(dc, logstd, N.STEPS[0])):
        assert torch.equal(_bits(x), _bits(y))
    assert bool((runs[0][3] != runs[1][3]).all()) and torch.equal(_bits(runs[0][2]), _bits(runs[1][2]))
    assert len(np.unique(runs[0][3].cpu().numpy())) == E * D


def test_the_moments_of_8192_draws():
    """E = 4096, D = 2, n = 8192: mean within 5 / sqrt(n), variance within 5 sqrt(2 / n) of 1, correlation of the two components
    within 5 / sqrt(n).  The NumPy restatement of the same draws meets the bounds at this key (checked on the CPU before they
    were fixed): mean 1.6e-3, variance 1.0263, correlation 3.5e-3 against 0.0552, 0.0781 and 0.0552."""
    case = N.Case("moments")
    eps = N.launch(A.DeviceCase(case), case.logstd.cuda(), N.STEPS[0])[3].cpu().numpy().astype(np.float64)
    n, corr = eps.size, float(np.corrcoef(eps[:, 0], eps[:, 1])[0, 1])
    print("FIGURE mean %.4g variance %.5g correlation %.4g" % (eps.mean(), eps.var(), corr))
    assert n == 8192 and abs(eps.mean()) <= 5 / np.sqrt(n) and abs(eps.var() - 1.0) <= 5 * np.sqrt(2.0 / n) and abs(corr) <= 5 / np.sqrt(n)


def test_refusals_come_before_any_launch():
    from rltime_amd._lib import lib
    w = (C.c_int32 * 2)(64, 0)
    assert [lib.mirl_act_mlp_normal_supported(16, 2, 1, w, 64, d) for d in (0, 1, 16, 17)] == [0, 1, 1, 0]
    for D, pitch in ((1, 2), (17, 2)):           # null operands (logstd and the step word among them); D = 17
        assert lib.mirl_act_mlp_normal_fwd(16, 2, 1, w, 64, D, *[None] * 10, 0, None, None, None, pitch, None, None, None) < 0
