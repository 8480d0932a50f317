"""The acting network of csrc/act_mlp.hip (mirl_act_mlp_fwd) restated layer by layer in torch at a chosen precision, the test
shapes with their seeded operands, and the launch through the C-ABI.  Reference order: rltime/policies/torch/dqn.py:50-87,
132-148, iqn.py:67-131.  Used by tests/test_fused_mlp_cpu.py (the float64 reference alone: are the seeds' rows clear?),
tests/test_act_mlp_gpu.py and tests/test_fused_mlp_step_gpu.py."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

# (E, O, widths, N, D, HID, A, dueling): the smallest shapes that reach each branch of the kernel
SHAPES = {
    "shipped-iqn": (16, 4, [64], 32, 64, 128, 2, True),
    "shipped-dqn": (16, 4, [64], 1, 0, 64, 2, False),
    "no-wave-multiple": (3, 5, [24], 5, 16, 40, 3, False),
    "no-leading-layer": (2, 7, [], 4, 8, 33, 3, True),
    "every-limit": (1, 64, [256, 256], 64, 64, 512, 32, True),
    "dueling-dqn": (5, 4, [64], 1, 0, 128, 2, True),
}
# seeds for which the float64 reference leaves at most one row in eight with a top-two gap <= 1e-4
# (tests/test_fused_mlp_cpu.py::test_the_seeds_leave_clear_rows checks that without a GPU)
SEEDS = {"shipped-iqn": 1, "shipped-dqn": 2, "no-wave-multiple": 3, "no-leading-layer": 4, "every-limit": 5, "dueling-dqn": 6}
CLEAR = 1e-4


class Case:
    """The operands of one launch, on the CPU, in the layouts the policy holds them: Linear weights (out, in)."""

    def __init__(self, name):
        self.name = name
        self.E, self.O, self.widths, self.N, self.D, self.HID, self.A, self.dueling = SHAPES[name]
        g = torch.Generator().manual_seed(SEEDS[name])
        rn = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
        E, O, N, D, HID, A = self.E, self.O, self.N, self.D, self.HID, self.A
        self.obs = rn(E, O) * 0.7
        self.leading, k = [], O
        for w in self.widths:
            self.leading.append((rn(w, k) / math.sqrt(k), rn(w) * 0.1))
            k = w
        W = self.W = k
        self.NO = A + (1 if self.dueling else 0)
        self.h1 = HID - HID // 2 if self.dueling else HID       # [last FC | value-hidden]
        self.taus = torch.rand(E * N, generator=g) if D else None
        self.freq = (torch.arange(1, D + 1, dtype=torch.float32) * math.pi) if D else None
        self.wq, self.bq = (rn(W, D) / math.sqrt(D), rn(W) * 0.1) if D else (None, None)
        self.wfc, self.bfc = rn(HID, W) / math.sqrt(W), rn(HID) * 0.1
        wout = rn(self.NO, HID) / math.sqrt(self.h1)
        if self.dueling:                                        # block-diagonal: advantages read the FC's units, the value its own
            wout[:A, self.h1:] = 0.0
            wout[A:, :self.h1] = 0.0
        self.wout, self.bout = wout, rn(self.NO) * 0.1

    def shape_args(self):
        """(E, O, L, widths, N, D, HID, NO, A) as mirl_act_mlp_supported takes them."""
        widths = (C.c_int32 * 2)(*(list(self.widths) + [0, 0])[:2])
        return (self.E, self.O, len(self.widths), widths, self.N, self.D, self.HID, self.NO, self.A)


def reference(case, dtype, taus=None, device="cpu"):
    """-> (q [E][A], advantage means [E][A]) at `dtype` on `device`; taus default to the case's."""
    c = case
    to = lambda t: t.to(device=device, dtype=dtype)             # noqa: E731
    f = to(c.obs)
    for w, b in c.leading:
        f = F.relu(F.linear(f, to(w), to(b)))
    x = f.repeat_interleave(c.N, dim=0)
    if c.D:
        taus = c.taus if taus is None else taus
        phi = torch.cos(to(c.freq) * to(taus).unsqueeze(1))
        x = F.relu(F.linear(phi, to(c.wq), to(c.bq))) * x
    hid = F.relu(F.linear(x, to(c.wfc), to(c.bfc)))
    out = F.linear(hid, to(c.wout), to(c.bout))
    adv = out[:, :c.A]
    q = out[:, c.A:c.A + 1] + adv - adv.mean(1, keepdim=True) if c.dueling else adv
    return q.reshape(c.E, c.N, c.A).mean(1), adv.reshape(c.E, c.N, c.A).mean(1)


def clear_rows(q64):
    """Rows whose float64 top-two gap exceeds CLEAR (all rows when there is one action)."""
    if q64.shape[1] < 2:
        return torch.ones(q64.shape[0], dtype=torch.bool, device=q64.device)
    top2 = q64.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > CLEAR


def check_bar(got, want64, lib32, floor=5e-6):
    """tests/test_actnet_gpu.py::test_head's bar: |got - f64| <= max(4 x max|torch f32 - f64|, floor x max(scale, 1)).
    -> (err, ref, scale) for the caller to print."""
    scale = float(want64.abs().max())
    err = float((got.double() - want64).abs().max())
    ref = float((lib32.double() - want64).abs().max())
    assert err <= max(4 * ref, floor * max(scale, 1.0)), (err, ref, scale)
    return err, ref, scale


class DeviceCase:
    """The case's operands on the GPU in the kernel's layouts: every weight transposed, [K][J] row-major."""

    def __init__(self, case, device="cuda"):
        c = self.case = case
        d = lambda t: None if t is None else t.to(device).contiguous()          # noqa: E731
        t = lambda w: None if w is None else w.t().contiguous().to(device)      # noqa: E731
        self.obs = d(c.obs)
        self.lwT = [t(w) for w, _ in c.leading] + [None, None]
        self.lb = [d(b) for _, b in c.leading] + [None, None]
        self.freq, self.taus, self.wqT, self.bq = d(c.freq), d(c.taus), t(c.wq), d(c.bq)
        self.fcT, self.fcb, self.outT, self.outb = t(c.wfc), d(c.bfc), t(c.wout), d(c.bout)
        self.device = device

    def launch(self, taus="given", need_q=1, eps=None, seed=99, step=5, actions=None, qvalues=None, taus_out=None):
        """One mirl_act_mlp_fwd launch -> (actions int32 [E], qvalues [E][A]).  taus: "given" (the case's), None (drawn in
        the kernel) or a tensor; eps: None (greedy) or a float."""
        from rltime_amd._lib import lib, check
        c = self.case
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(None)     # noqa: E731
        if isinstance(taus, str):
            taus = self.taus
        self.step = torch.tensor([step], dtype=torch.int64, device=self.device)
        self.eps = torch.tensor(eps, dtype=torch.float64, device=self.device) if eps is not None else None
        actions = torch.full((c.E,), -1, dtype=torch.int32, device=self.device) if actions is None else actions
        qvalues = torch.full((c.E, c.A), float("nan"), device=self.device) if qvalues is None else qvalues
        check(lib.mirl_act_mlp_fwd(
            *c.shape_args(), c.h1, need_q, p(self.obs), p(self.lwT[0]), p(self.lb[0]), p(self.lwT[1]), p(self.lb[1]),
            p(self.freq), p(taus), p(self.wqT), p(self.bq), p(self.fcT), p(self.fcb), p(self.outT), p(self.outb),
            p(self.eps), None, 0.0, seed, p(self.step), p(actions), p(qvalues), p(taus_out),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mirl_act_mlp_fwd")
        return actions, qvalues


# ---- a float64 copy of a policy (DQNPolicy / IQNPolicy over FC modules) for the step tests -------------------------------------------
def policy_q64(pol, obs, taus=None):
    """The policy's q-values [E][A] in float64 on the CPU from its state dict: FC modules, quantile product before the last
    one, the last FC module, the output layer, the dueling combine, the mean over the quantile rows."""
    sd = {k: v.detach().double().cpu() for k, v in pol.state_dict().items()}
    lin = lambda x, name: x @ sd[name + ".weight"].t() + sd[name + ".bias"]      # noqa: E731
    layers = len(pol.model.layers)
    x = obs.detach().double().cpu()
    E = x.shape[0]
    for i in range(layers - 1):
        x = F.relu(lin(x, "model.layers.%d.layers.0.0" % i))
    N = 1
    if "quantile_layer.weight" in sd:
        N = pol.num_sampling_quantiles
        freq = (sd["embedding_range"].float() * math.pi).double()               # the float32 frequencies the kernels read
        phi = torch.cos(freq * taus.detach().double().cpu().unsqueeze(1))
        x = F.relu(lin(phi, "quantile_layer")) * x.repeat_interleave(N, dim=0)
    adv = lin(F.relu(lin(x, "model.layers.%d.layers.0.0" % (layers - 1))), "out_layer")
    q = adv
    if "value_layer.weight" in sd:
        val = lin(F.relu(lin(x, "value_hidden_layer")), "value_layer")
        q = val + adv - adv.mean(1, keepdim=True)
    return q.reshape(E, N, -1).mean(1)
