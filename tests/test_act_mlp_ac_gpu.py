"""GPU: csrc/act_mlp.hip k_act_mlp<true> — the whole acting network of an actor-critic MLP policy with its sampling head in one
launch (mirl_act_mlp_ac_fwd) — through the C-ABI:

  1. logits_out against the float64 evaluation of the same layers, within the bar mirl_act_mlp_fwd is held to (R.check_bar);
  2. logits_out against mirl_act_mlp_fwd on the same weights as a plain head of A + 1 "actions", bit for bit: the product path
     inherits the float64 pinning of tests/test_act_mlp_exact_gpu.py;
  3. the head against mirl_actor_head_ac_rng fed logits_out at the same key, bit for bit, sampled and greedy, two step words;
  4. the evaluation's epsilon remap against the NumPy restatement on Philox words 2 and 3;
  5. a rerun, guard words around every output, and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import act_mlp_ac_restate as A
from tests import act_mlp_restate as R

pytestmark = pytest.mark.gpu

NAMES = sorted(A.SHAPES)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case on the device with its references, computed once: float64 and torch's float32 on the GPU, and one sampled
    launch at the first step word."""
    case = A.Case(name)
    dc = A.DeviceCase(case)
    out64 = A.reference(case, torch.float64, device="cuda")
    out32 = A.reference(case, torch.float32, device="cuda")
    return case, dc, out64, out32


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", NAMES)
def test_logits_out_matches_float64(name):
    case, dc, out64, out32 = _case(name)
    actions, policy, logits = dc.launch()
    print(name, "err, torch f32 err, scale:", R.check_bar(logits, out64, out32))
    assert torch.equal(_bits(policy[:, 1]), _bits(logits[:, case.A]))              # the value is the product's last column
    assert int(actions.min()) >= 0 and int(actions.max()) < case.A and bool(torch.isfinite(policy).all())


@pytest.mark.parametrize("name", [n for n in NAMES if A.SHAPES[n][4] + 1 <= 32])
def test_logits_out_is_act_mlp_fwds_product_to_the_bit(name):
    case, dc, _, _ = _case(name)
    _, _, logits = dc.launch()
    q = dc.launch_q()
    assert torch.equal(_bits(q), _bits(logits))


@pytest.mark.parametrize("greedy", [0, 1])
@pytest.mark.parametrize("step", A.STEPS)
@pytest.mark.parametrize("name", NAMES)
def test_the_head_is_actor_head_ac_rngs(name, step, greedy):
    from rltime_amd._lib import lib, check
    case, dc, _, _ = _case(name)
    E, NA = case.E, case.A
    actions, policy, logits = dc.launch(step=step, greedy=greedy)
    want_a = torch.full((E,), -1, dtype=torch.int32, device="cuda")
    want_p = torch.full((E, 2), float("nan"), device="cuda")
    word = torch.tensor([step], dtype=torch.int64, device="cuda")
    check(lib.mirl_actor_head_ac_rng(E, NA, _p(logits), NA + 1, C.c_void_p(logits.data_ptr() + 4 * NA), NA + 1, A.RNG_SEED, _p(word),
                                     greedy, _p(want_a), _p(want_p), C.c_void_p(want_p.data_ptr() + 4), 2, _st()),
          "mirl_actor_head_ac_rng")
    assert torch.equal(actions, want_a) and torch.equal(_bits(policy), _bits(want_p))
    # and the restatement on the same rows: the actions wherever the uniform is clear of a CDF boundary, the log-probability
    # within its one rounding
    from tests import actor_critic_restate as AR
    rows = logits.cpu().numpy()
    ra, rlp, rv = A.head(rows, A.RNG_SEED, step, greedy=bool(greedy))
    if greedy:
        assert np.array_equal(actions.cpu().numpy(), ra)
    else:
        u = A.uniform24(A.philox_words(A.RNG_SEED, step, E)[:, 0])
        margin, bound = AR.head_margin(rows[:, :NA].astype(np.float64), u)
        clear = margin > bound
        assert clear.all(), "a uniform on a CDF boundary: pick another seed"
        assert np.array_equal(actions.cpu().numpy(), ra)
    assert np.all(np.abs(policy[:, 0].double().cpu().numpy() - rlp) <= AR.head_logp_bound(rlp))
    assert np.array_equal(policy[:, 1].cpu().numpy(), rv)
    if NA == 1:
        assert bool((actions == 0).all()) and bool((policy[:, 0] == 0).all())


@pytest.mark.parametrize("name", NAMES)
def test_the_eps_remap_is_the_restatements(name):
    case, dc, _, _ = _case(name)
    E, NA = case.E, case.A
    for step in A.STEPS:
        sampled, policy0, _ = dc.launch(step=step)
        for eps in (1.0, 0.0, 0.5):
            got, policy, _ = dc.launch(step=step, eps=eps)
            want, near = A.eps_remap(sampled.cpu().numpy(), A.RNG_SEED, step, NA, eps)
            assert not near.any()
            assert np.array_equal(got.cpu().numpy(), want), (step, eps)
            assert torch.equal(_bits(policy), _bits(policy0))     # the log-probability stays the sampled action's
        # per-actor exponents and a floor, and the remap under greedy (the block is drawn for the remap alone)
        expo = torch.arange(1, E + 1, dtype=torch.float64, device="cuda")
        got, _, _ = dc.launch(step=step, eps=0.5, expo=expo, eps_min=0.1)
        want, near = A.eps_remap(sampled.cpu().numpy(), A.RNG_SEED, step, NA, 0.5, expo=expo.cpu().numpy(), eps_min=0.1)
        assert not near.any() and np.array_equal(got.cpu().numpy(), want)
        first, _, _ = dc.launch(step=step, greedy=1)
        got, _, _ = dc.launch(step=step, greedy=1, eps=1.0)
        want, _ = A.eps_remap(first.cpu().numpy(), A.RNG_SEED, step, NA, 1.0)
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", NAMES)
def test_a_rerun_repeats_and_nothing_is_written_past_the_outputs(name):
    case, dc, _, _ = _case(name)
    E, NO, pad = case.E, case.NO, 64
    a1, p1, l1 = dc.launch()
    a2, p2, l2 = dc.launch()
    assert torch.equal(a1, a2) and torch.equal(_bits(p1), _bits(p2)) and torch.equal(_bits(l1), _bits(l2))
    # guard words before and after each output
    abuf = torch.full((pad + E + pad,), -7, dtype=torch.int32, device="cuda")
    pbuf = torch.full((pad + 2 * E + pad,), -7.0, device="cuda")
    lbuf = torch.full((pad + E * NO + pad,), -7.0, device="cuda")
    dc.launch(actions=abuf[pad:pad + E], policy=pbuf[pad:pad + 2 * E], logits_out=lbuf[pad:pad + E * NO])
    assert torch.equal(abuf[pad:pad + E], a1) and torch.equal(_bits(pbuf[pad:pad + 2 * E]), _bits(p1).flatten())
    assert torch.equal(_bits(lbuf[pad:pad + E * NO]), _bits(l1).flatten())
    for buf, n in ((abuf, E), (pbuf, 2 * E), (lbuf, E * NO)):
        assert bool((buf[:pad] == -7).all()) and bool((buf[pad + n:] == -7).all())
    # a wider pitch: the columns past the pair stay untouched; logits_out NULL: the same actions and pair
    wide = torch.full((E, 5), -7.0, device="cuda")
    a3, _, none = dc.launch(policy=wide, out_pitch=5, logits_out=None)
    assert none is None and torch.equal(a3, a1) and torch.equal(_bits(wide[:, :2]), _bits(p1)) and bool((wide[:, 2:] == -7).all())


def test_every_refusal_leaves_the_outputs_untouched():
    from rltime_amd._lib import lib, MIRL_ERR_ARG
    case, dc, _, _ = _case("shipped")
    E, NO = case.E, case.NO
    abuf = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    pbuf = torch.full((E, 2), -7.0, device="cuda")
    lbuf = torch.full((E, NO), -7.0, device="cuda")
    names = ["E", "O", "L", "widths", "HID", "A", "obs", "lw0T", "lb0", "lw1T", "lb1", "fcT", "fcb", "outT", "outb", "eps", "expo",
             "eps_min", "seed", "step", "greedy", "actions", "policy", "out_pitch", "logits_out", "stream"]

    def call(**kw):
        args, _ = dc.args(A.RNG_SEED, 5, greedy=kw.pop("greedy", 0), actions=abuf, policy=pbuf, logits_out=lbuf)
        assert len(args) == len(names)
        named = dict(zip(names, args))
        named.update(kw)
        return lib.mirl_act_mlp_ac_fwd(*named.values())

    null = C.c_void_p(None)
    refusals = [dict(O=65), dict(O=0), dict(HID=513), dict(A=33), dict(A=0), dict(E=0), dict(L=3), dict(widths=(C.c_int32 * 2)(257, 0)),
                dict(widths=None), dict(greedy=2), dict(out_pitch=1), dict(step=null), dict(step=null, greedy=1)]
    refusals += [{key: null} for key in ("obs", "lw0T", "lb0", "fcT", "fcb", "outT", "outb", "actions", "policy")]
    refusals += [dict(L=2, widths=(C.c_int32 * 2)(64, 64))]       # a second leading layer without its operands
    for kw in refusals:
        assert call(**dict(kw)) == MIRL_ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((abuf == -7).all()) and bool((pbuf == -7).all()) and bool((lbuf == -7).all())
    assert call() == 0                                            # the same list unchanged is taken
    torch.cuda.synchronize()
    assert bool((abuf != -7).all()) and bool((pbuf != -7).all()) and bool((lbuf != -7).all())
