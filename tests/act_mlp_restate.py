"""The acting network of csrc/act_mlp.hip (mirl_act_mlp_fwd) restated layer by layer in torch at a chosen precision, the test
shapes with their seeded operands, and the launch through the C-ABI.  Reference order: rltime/policies/torch/dqn.py:50-87,
132-148, iqn.py:67-131.  Used by tests/test_fused_mlp_cpu.py (the float64 reference alone: are the seeds' rows clear?),
tests/test_act_mlp_gpu.py and tests/test_fused_mlp_step_gpu.py.

For tests/test_act_mlp_exact_gpu.py and tests/test_act_mlp_restate_cpu.py: the shapes that reach the remaining branches of
`dense_rb` with the host arithmetic that names the branch a launch takes, the float64 walk product by product with the
first-order bound of the kernel's float32 arithmetic, a NumPy float32 restatement of that arithmetic, and dyadic operands on
which every sum is exact and every row's maximum is tied."""
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

# the smallest shapes that reach the branches of `dense_rb` and of the head that the six above leave out; what each one
# reaches is asserted by `assert_branches` (kept apart from SHAPES: the tests over SHAPES run as they did)
BRANCH_SHAPES = {
    "two-row-passes": (8, 6, [200], 27, 16, 96, 3, True),
    "ragged-chunks-of-16": (8, 5, [40, 256], 40, 64, 300, 9, True),
    "ragged-chunk-of-32": (8, 5, [24], 37, 8, 40, 3, False),
    "hid-192": (8, 4, [150], 8, 12, 384, 12, True),
    "plain-observation": (8, 7, [], 1, 0, 33, 3, False),
    "one-action": (8, 4, [64], 4, 8, 64, 1, True),
    "many-envs": (300, 4, [64], 1, 0, 64, 2, False),
}
# seeds for which at most one row in eight has its two best float64 q-values closer than the sum of their two bounds
# (tests/test_act_mlp_restate_cpu.py::test_the_seeds_leave_rows_clear_of_their_bounds)
BRANCH_SEEDS = {"two-row-passes": 1, "ragged-chunks-of-16": 2, "ragged-chunk-of-32": 3, "hid-192": 1, "plain-observation": 2,
                "one-action": 3, "many-envs": 1}
ALL_SHAPES = {**SHAPES, **BRANCH_SHAPES}
ALL_SEEDS = {**SEEDS, **BRANCH_SEEDS}
U = 2.0 ** -24


class Dims:
    """The sizes of one launch.  dueling: None (the shape's own) or the twin with / without a value stream."""

    def __init__(self, name, dueling=None):
        self.name = name
        self.E, self.O, self.widths, self.N, self.D, self.HID, self.A, self.dueling = ALL_SHAPES[name]
        if dueling is not None:
            self.dueling = dueling
        self.W = self.widths[-1] if self.widths else self.O
        self.NO = self.A + (1 if self.dueling else 0)
        self.h1 = self.HID - self.HID // 2 if self.dueling else self.HID        # [last FC | value-hidden]

    def shape_args(self):
        """(E, O, L, widths, N, D, HID, NO, A) as mirl_act_mlp_supported takes them."""
        widths = (C.c_int32 * 2)(*(list(self.widths) + [0, 0])[:2])
        return (self.E, self.O, len(self.widths), widths, self.N, self.D, self.HID, self.NO, self.A)


class Case(Dims):
    """The operands of one launch, on the CPU, in the layouts the policy holds them: Linear weights (out, in)."""

    def __init__(self, name):
        super().__init__(name)
        g = torch.Generator().manual_seed(ALL_SEEDS[name])
        rn = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
        E, O, N, D, HID, A = self.E, self.O, self.N, self.D, self.HID, self.A
        self.obs = rn(E, O) * 0.7
        self.leading, k = [], O
        for w in self.widths:
            self.leading.append((rn(w, k) / math.sqrt(k), rn(w) * 0.1))
            k = w
        W = self.W
        self.taus = torch.rand(E * N, generator=g) if D else None
        self.freq = (torch.arange(1, D + 1, dtype=torch.float32) * math.pi) if D else None
        self.wq, self.bq = (rn(W, D) / math.sqrt(D), rn(W) * 0.1) if D else (None, None)
        self.wfc, self.bfc = rn(HID, W) / math.sqrt(W), rn(HID) * 0.1
        wout = rn(self.NO, HID) / math.sqrt(self.h1)
        if self.dueling:                                        # block-diagonal: advantages read the FC's units, the value its own
            wout[:A, self.h1:] = 0.0
            wout[A:, :self.h1] = 0.0
        self.wout, self.bout = wout, rn(self.NO) * 0.1


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

    def launch(self, taus="given", need_q=1, eps=None, seed=99, step=5, actions=None, qvalues=None, taus_out=None, expo=None,
               eps_min=0.0):
        """One mirl_act_mlp_fwd launch -> (actions int32 [E], qvalues [E][A]).  taus: "given" (the case's), None (drawn in
        the kernel) or a tensor; eps: None (greedy) or a float; expo: None or a float64 tensor [E] on the device."""
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
            p(self.eps), p(expo), float(eps_min), seed, p(self.step), p(actions), p(qvalues), p(taus_out),
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


# ---- the launch geometry: which branches of dense_rb a shape takes ----------------------------------------------------------------
TILE = 4096                                  # ACT_MLP_TILE


def dense_geometry(RB, R, K, J):
    """dense_rb<RB>(R rows, K inputs, J units) as csrc/act_mlp.hip lays it out: JP lanes per row group, G row groups, one
    column pass per JP units (Jt wide, whole k rows of the 4096-float tile: TK of them, `tiles` rows per fetch) and one row
    pass per G RB rows."""
    JP = 256 if J >= 256 else (J + 63) & ~63
    G = 256 // JP
    passes = []
    for j0 in range(0, J, JP):
        Jt = min(J - j0, JP)
        TK = TILE // Jt
        passes.append({"j0": j0, "Jt": Jt, "TK": TK, "tiles": [min(K - k0, TK) for k0 in range(0, K, TK)]})
    return {"RB": RB, "R": R, "K": K, "J": J, "JP": JP, "G": G, "passes": passes, "row_passes": list(range(0, R, G * RB)),
            "idle_waves": 4 - G * JP // 64}


def chunk_rows(dims):
    """-> (CH, dynamic LDS bytes): mirl_act_mlp_lds_bytes (host logic) solved for CH in
    4 (2 x 256 + 64 + 4096 + CH (D + W + HID) + N NO)."""
    from rltime_amd._lib import lib
    need = C.c_int64()
    assert lib.mirl_act_mlp_lds_bytes(*dims.shape_args()[1:], C.byref(need)) == 0
    rest, per_row = need.value - 4 * (576 + TILE + dims.N * dims.NO), 4 * (dims.D + dims.W + dims.HID)
    assert rest > 0 and rest % per_row == 0, (need.value, per_row)
    return rest // per_row, need.value


def launch_geometry(dims, need_q):
    """The five products of one launch as the kernel runs them: the leading layers, then per chunk of CH quantile rows the
    quantile product, the last FC [+ value-hidden] and the output layer."""
    CH, lds = chunk_rows(dims)
    full = bool(need_q) or not dims.dueling
    hid_run, no_run = (dims.HID, dims.NO) if full else (dims.h1, dims.A)
    chunks = [(n0, min(dims.N - n0, CH)) for n0 in range(0, dims.N, CH)]
    RB = 16 if dims.D else 1
    lead, k = [], dims.O
    for w in dims.widths:
        lead.append(dense_geometry(1, 1, k, w))
        k = w
    return {"CH": CH, "lds": lds, "chunks": chunks, "hid_run": hid_run, "no_run": no_run, "lead": lead,
            "quant": [dense_geometry(16, R, dims.D, dims.W) for _, R in chunks] if dims.D else [],
            "fc": [dense_geometry(RB, R, dims.W, hid_run) for _, R in chunks],
            "out": [dense_geometry(RB, R, hid_run, no_run) for _, R in chunks]}


def assert_branches(name):
    """The branch each shape of BRANCH_SHAPES is there for, from the launcher's own chunk size: a shape whose geometry is not
    what its name says fails here, in the GPU case that launches it and in the CPU test."""
    d = Dims(name)
    g1, g0 = launch_geometry(d, 1), launch_geometry(d, 0)
    tiles = lambda p: [t["tiles"] for t in p["passes"]]          # noqa: E731
    widths = lambda p: [t["Jt"] for t in p["passes"]]            # noqa: E731
    if name in SHAPES:
        # the six earlier shapes: one row pass everywhere (what the branch shapes are there to leave); every-limit alone has
        # the LDS limit raised
        assert all(len(p["row_passes"]) == 1 for g in (g1, g0) for k in ("lead", "quant", "fc", "out") for p in g[k])
        assert (g1["lds"] > 65536) == (name == "every-limit")
        return g1, g0
    assert g1["lds"] == g0["lds"] <= 65536, "no new shape raises the LDS limit"
    if name == "two-row-passes":
        q = g1["quant"]
        assert g1["CH"] == 32 and g1["chunks"] == [(0, 27)] and len(q) == 1
        assert q[0]["JP"] == 256 and q[0]["G"] == 1 and q[0]["row_passes"] == [0, 16] and q[0]["R"] - 16 == 11      # 11 live, 5 clamped
        assert g1["fc"][0]["G"] == 2 and g1["fc"][0]["row_passes"] == [0]
        assert g0["fc"][0]["J"] == 48 and g0["out"][0]["K"] == 48
    elif name == "ragged-chunks-of-16":
        assert g1["CH"] == 16 and g1["chunks"] == [(0, 16), (16, 16), (32, 8)]                # n0 > 0 with R < CH
        assert widths(g1["fc"][0]) == [256, 44] and g1["fc"][0]["passes"][1]["TK"] == 93 and tiles(g1["fc"][0])[1] == [93, 93, 70]
        assert d.widths[0] != d.widths[1] and g1["lead"][1]["K"] == 40 and tiles(g1["lead"][1]) == [[16, 16, 8]]    # K % 16 != 0 at Jt = 256
        assert d.A == 9 and 33 <= d.N <= 63
        f0 = g0["fc"][0]
        assert f0["J"] == 150 and f0["JP"] == 192 and f0["G"] == 1 and f0["idle_waves"] == 1 and g0["out"][0]["K"] == 150
    elif name == "ragged-chunk-of-32":
        assert g1["CH"] == 32 and g1["chunks"] == [(0, 32), (32, 5)] and 33 <= d.N <= 63
        assert g1["quant"][0]["G"] == 4 and g1["quant"][0]["row_passes"] == [0]
    elif name == "hid-192":
        for p in (g1["lead"][0], g1["quant"][0]):
            assert p["J"] == 150 and p["JP"] == 192 and p["G"] == 1 and p["idle_waves"] == 1
        assert widths(g1["fc"][0]) == [256, 128] and g1["fc"][0]["passes"][1]["TK"] == 32
        assert g0["fc"][0]["J"] == 192 == g0["fc"][0]["JP"] and 9 <= d.A <= 31 and d.A % 8
    elif name == "plain-observation":
        assert not d.widths and d.D == 0 and g1["lead"] == [] and g1["quant"] == [] and g1["fc"][0]["K"] == d.O and g1["fc"][0]["RB"] == 1
    elif name == "one-action":
        assert d.A == 1 and d.NO == 2 and g1["out"][0]["J"] == 2 and g0["out"][0]["J"] == 1
    elif name == "many-envs":
        assert d.E > 256                                           # more workgroups than the chip has compute units
    else:
        raise AssertionError("no branch recorded for " + name)
    return g1, g0


# ---- float64 in the kernel's product structure, with the first-order bound of its float32 arithmetic ---------------------------
def _dense64(x, e_x, w, b):
    """y = x w^T + b in float64 and the bound of the kernel's float32 value of it: s_j = sum_k x_k w_kj is added in ascending k
    from 0 with one multiply and one add per term, K roundings at most on any term: e_s = sum_k |w_kj| e_x,k + K u sum_k
    |x_k w_kj|; the bias addition rounds once: + u |s + b|."""
    K = x.shape[1]
    aw = w.abs().t()
    y = x @ w.t() + b
    return y, e_x @ aw + K * U * (x.abs() @ aw) + U * y.abs()


def forward_bound(case, need_q=1, phi=None):
    """The network in float64, product by product as mirl_act_mlp_fwd runs them (need_q = 0 under a dueling head: the
    advantage stream alone), and per output the first-order bound (u = 2^-24) of the kernel's float32 result.  phi: the
    cosine features (E N, D) as float32 numbers, taken as exact (default: torch's float32 cos of the float32 product).
    ReLU is 1-Lipschitz: a bound passes through it unchanged.  Feature product x = r f: |f| e_r + |r| e_f + u |x|.  Head (the
    `actor head` row of docs/parity.md with one row per lane, on top of the propagated bound of the output layer):
    off = V - m / A: e_off = e_V + sum_a e_a / A + u ((A - 1) sum_a |A_a| / A + |m| / A + |off|); t = A_a + off: e_t = e_a + e_off + u |t|
    (no value stream: t = A_a, e_t = e_a); q = sum_n t / N: e_q = (sum_n e_t + 7 u sum_n |t|) / N + u |q|.
    -> dict(q (E, A), bound (E, A), products [(name, x, w, b)] as launched)."""
    c = case
    d = lambda t: t.double()                                       # noqa: E731
    relu = lambda t: torch.clamp(t, min=0)                         # noqa: E731
    full = bool(need_q) or not c.dueling
    products = []
    f, e_f = d(c.obs), torch.zeros(c.E, c.O, dtype=torch.float64)
    for i, (w, b) in enumerate(c.leading):
        products.append(("lead%d" % i, f, d(w), d(b)))
        y, e_f = _dense64(f, e_f, d(w), d(b))
        f = relu(y)
    x, e_x = f.repeat_interleave(c.N, dim=0), e_f.repeat_interleave(c.N, dim=0)
    if c.D:
        if phi is None:
            phi = torch.cos(c.freq * c.taus.unsqueeze(1))
        assert phi.dtype == torch.float32 and phi.shape == (c.E * c.N, c.D)
        phi = d(phi)
        products.append(("quant", phi, d(c.wq), d(c.bq)))
        y, e_r = _dense64(phi, torch.zeros_like(phi), d(c.wq), d(c.bq))
        r = relu(y)
        e_x = x.abs() * e_r + r * e_x
        x = r * x
        e_x = e_x + U * x.abs()
    hid_run, no_run = (c.HID, c.NO) if full else (c.h1, c.A)
    wfc, bfc = d(c.wfc)[:hid_run], d(c.bfc)[:hid_run]
    products.append(("fc", x, wfc, bfc))
    y, e_h = _dense64(x, e_x, wfc, bfc)
    hid = relu(y)
    wout, bout = d(c.wout)[:no_run, :hid_run], d(c.bout)[:no_run]
    products.append(("out", hid, wout, bout))
    out, e_o = _dense64(hid, e_h, wout, bout)
    A = c.A
    t, e_t = out[:, :A], e_o[:, :A]
    if c.dueling and full:
        m = t.sum(1, keepdim=True)
        off = out[:, A:A + 1] - m / A
        e_off = e_o[:, A:A + 1] + e_t.sum(1, keepdim=True) / A + U * ((A - 1) * t.abs().sum(1, keepdim=True) / A + m.abs() / A + off.abs())
        t = t + off
        e_t = e_t + e_off + U * t.abs()
    t, e_t = t.reshape(c.E, c.N, A), e_t.reshape(c.E, c.N, A)
    q = t.sum(1) / c.N
    bound = (e_t.sum(1) + 7 * U * t.abs().sum(1)) / c.N + U * q.abs()
    return {"q": q, "bound": bound, "t": t, "products": products}


def first_max(q):
    """First maximum per row (numpy.argmax)."""
    return torch.from_numpy(q.numpy().argmax(1))


def allowed_actions(q, bound):
    """-> (best (E,), other (E,), close (E,) bool): the float64 arg-max, and where the two best q-values are closer than the sum
    of their two bounds the second best, which the kernel may take instead."""
    E, A = q.shape
    best = first_max(q)
    if A < 2:
        return best, best.clone(), torch.zeros(E, dtype=torch.bool)
    top = q.topk(2, dim=1)
    rows = torch.arange(E)
    close = (top.values[:, 0] - top.values[:, 1]) <= bound[rows, top.indices[:, 0]] + bound[rows, top.indices[:, 1]]
    other = torch.where(top.indices[:, 0] == best, top.indices[:, 1], top.indices[:, 0])
    return best, other, close


def check_bound(got, fb, actions, label):
    """|got - float64| <= bound per element; the actions are the float64 arg-max, or on rows too close to call either of the
    two best, which at most one row in eight may be.  -> worst err / bound, printed for docs/parity.md."""
    q, bound = fb["q"], fb["bound"]
    err = (got.double() - q).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print("RATIO k_act_mlp %s: worst err / bound = %.4f" % (label, ratio))
    assert bool((err <= bound).all()), "%s: err / bound = %.3f at %s" % (label, ratio, (err > bound).nonzero()[:4].tolist())
    best, other, close = allowed_actions(q, bound)
    assert int(close.sum()) * 8 <= q.shape[0], "%s: %d rows too close to call: pick another seed" % (label, int(close.sum()))
    acts = actions.long()
    assert bool(((acts == best) | (close & (acts == other))).all()), (label, (acts != best).nonzero().flatten()[:8].tolist())
    return ratio


# ---- the kernel's float32 arithmetic restated in NumPy (the CPU test's stand-in for the GPU) -----------------------------------
def _dense32(x, w, b):
    import numpy as np
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k in range(x.shape[1]):                                     # ascending k, a rounded product, a rounded addition
        acc = acc + x[:, k:k + 1] * w[None, :, k]
    return acc + b[None, :]


def emulate32(case, need_q=1, phi=None):
    """mirl_act_mlp_fwd's arithmetic in NumPy float32, operation for operation: products in ascending k with a separate
    multiply and add, the head's sum over the actions in ascending order, one row per lane and the xor butterfly 32 .. 1 over
    the wave, one division by N, the first maximum.  -> (actions (E,), q (E, A) float32)."""
    import numpy as np
    c = case
    n = lambda t: t.float().numpy()                                # noqa: E731
    relu = lambda a: np.maximum(a, np.float32(0))                  # noqa: E731
    full = bool(need_q) or not c.dueling
    f = n(c.obs)
    for w, b in c.leading:
        f = relu(_dense32(f, n(w), n(b)))
    x = np.repeat(f, c.N, axis=0)
    if c.D:
        if phi is None:
            phi = torch.cos(c.freq * c.taus.unsqueeze(1))
        x = relu(_dense32(n(phi), n(c.wq), n(c.bq))) * x
    hid_run, no_run = (c.HID, c.NO) if full else (c.h1, c.A)
    hid = relu(_dense32(x, n(c.wfc)[:hid_run], n(c.bfc)[:hid_run]))
    out = _dense32(hid, n(c.wout)[:no_run, :hid_run], n(c.bout)[:no_run])
    A, N = c.A, c.N
    off = np.zeros((out.shape[0], 1), np.float32)
    if c.dueling and full:
        m = np.zeros(out.shape[0], np.float32)
        for a in range(A):
            m = m + out[:, a]
        off = (out[:, A] - m / np.float32(A))[:, None]
    t = (out[:, :A] + off).reshape(c.E, N, A)
    lanes = np.zeros((c.E, A, 64), np.float32)
    lanes[:, :, :N] = t.transpose(0, 2, 1)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, :, idx ^ o]
    q = lanes[:, :, 0] / np.float32(N)
    assert q.dtype == np.float32
    return torch.from_numpy(q.argmax(1)), torch.from_numpy(q)


# ---- dyadic operands: every sum exact, every row's maximum tied -----------------------------------------------------------------
_VALUES = torch.tensor([-2.0, -1.0, -1.0, 1.0, 1.0, 1.0, 2.0])


def _pick(g, n):
    return _VALUES[torch.randint(0, len(_VALUES), (n,), generator=g)]


def _dyadic_weight(g, J, K, passes, per_unit=3):
    """(J, K) integers in {-2 .. 2}, sparse: per column pass (j0, Jt) every input k gets a non-zero weight in one unit of the
    pass, and every unit gets `per_unit` non-zero weights."""
    w = torch.zeros(J, K)
    ks = torch.arange(K)
    for j0, Jt in passes:
        w[j0 + torch.randint(0, Jt, (K,), generator=g), ks] = _pick(g, K)
    for j in range(J):
        sel = torch.randperm(K, generator=g)[:min(K, per_unit)]
        w[j, sel] = _pick(g, len(sel))
    return w


class DyadicCase(Dims):
    """Integer observations, sparse integer weights and biases, freq = 0 (cosf(0) = 1: the cosine features are exactly 1):
    every product, sum and the dueling mean (A a power of two) is exact in float32 in any order, and the mean over the N rows
    is one correctly rounded division of an exact sum, equal to the rounded float64 quotient (53 >= 2 x 24 + 2 bits).  The
    output layer has advantage column a copied to a + ceil(A / 2), weights and bias (an odd A's middle column is column 0 with
    the bias one lower): every row's maximum is tied and the first of the tied actions must win.  Every input k of every
    product has a non-zero weight in every column pass the launch makes (`coverage_gaps`), so that a dropped k, tile or pass
    changes a sum.  need_q = 1 takes the twin without a value stream where A is no power of two (m / A would round); need_q = 0
    never forms m / A and keeps the dueling layout, H1 columns at pitch HID."""

    def __init__(self, name, need_q):
        dueling = ALL_SHAPES[name][7]
        A = ALL_SHAPES[name][6]
        if need_q and dueling and A & (A - 1):
            dueling = False
        super().__init__(name, dueling=dueling)
        self.need_q = need_q
        g = torch.Generator().manual_seed(5000 + 2 * sorted(ALL_SHAPES).index(name) + need_q)
        ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()          # noqa: E731
        geo = launch_geometry(self, need_q)
        spans = lambda p: [(t["j0"], t["Jt"]) for t in p["passes"]]                          # noqa: E731
        E, O, N, D, HID, W = self.E, self.O, self.N, self.D, self.HID, self.W
        self.obs = ints(-2, 2, E, O)
        self.leading, k = [], O
        for i, w in enumerate(self.widths):
            self.leading.append((_dyadic_weight(g, w, k, spans(geo["lead"][i])), ints(-1, 2, w)))
            k = w
        self.taus = torch.rand(E * N, generator=g) if D else None
        self.freq = torch.zeros(D) if D else None
        self.wq, self.bq = (_dyadic_weight(g, W, D, spans(geo["quant"][0])), ints(0, 2, W)) if D else (None, None)
        run = geo["hid_run"]
        self.wfc = _dyadic_weight(g, HID, W, spans(geo["fc"][0]) + ([(run, HID - run)] if run < HID else []))
        self.bfc = ints(-1, 2, HID)
        h, h1 = (A + 1) // 2, self.h1
        wout, bout = torch.zeros(self.NO, HID), torch.zeros(self.NO)
        own = h - 1 if (A % 2 and A >= 3) else h                 # columns with weights of their own: they carry the coverage
        wout[:h, :h1], bout[:h] = _dyadic_weight(g, h, h1, [(0, own)]), ints(-2, 2, h)
        for a in range(h):
            if a + h < A:
                wout[a + h], bout[a + h] = wout[a], bout[a]
        if A % 2 and A >= 3:
            wout[h - 1], bout[h - 1] = wout[0], bout[0] - 1
        if self.dueling:
            wout[A, h1:] = torch.where(torch.rand(HID - h1, generator=g) < 0.5, -1.0, 1.0)
            bout[A] = float(ints(-2, 2, 1))
        self.wout, self.bout = wout, bout


def coverage_gaps(case, need_q):
    """[(product, pass start, inputs k without a non-zero weight in that pass)] over every product and column pass of the launch:
    empty when a dropped k, tile or pass must change a sum."""
    geo = launch_geometry(case, need_q)
    fb = forward_bound(case, need_q)
    launched = {"lead0": geo["lead"][0] if geo["lead"] else None, "lead1": geo["lead"][1] if len(geo["lead"]) > 1 else None,
                "quant": geo["quant"][0] if geo["quant"] else None, "fc": geo["fc"][0], "out": geo["out"][0]}
    gaps = []
    for name, x, w, _ in fb["products"]:
        p = launched[name]
        assert (p["K"], p["J"]) == (w.shape[1], w.shape[0]) == (x.shape[1], w.shape[0]), name
        for t in p["passes"]:
            missing = (~(w[t["j0"]:t["j0"] + t["Jt"]] != 0).any(0)).nonzero().flatten().tolist()
            if missing:
                gaps.append((name, t["j0"], missing))
    return gaps
