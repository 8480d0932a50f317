#!/usr/bin/env python3
"""Recorder for lstm_seq_parent.json: what the persistent LSTM sweeps (csrc/lstm_seq.hip) wrote, bit for bit, at the commit
BEFORE a refactor of that file.  Needs an MI355X and the built library; reads nothing outside the repository.

    python tests/golden/record_lstm_seq.py [output.json]

tests/test_lstm_seq_parent_gpu.py imports this module, launches the same cases on the tree under test and compares.

Inputs come from integer arithmetic, so any numpy reproduces them: element i of stream s is
((i * 2654435761 + s * 40503) mod 2^32) / 2^32, mapped per tensor (TENSORS below).  h0 spans +-3: a third of the initial state
has bit 30 of its float set and must travel the untagged, counter-guarded path unchanged.  Batches are fixed numbers; the
recorded form (narrow / wide) of every forward case is asserted through lds_bytes, on recording and on comparison.

Recorded: SHA-256 of the bytes of every output of mirl_lstm_seq_fwd (FWD_SHAPES x T in {1, 6} x save_gates in {0, 1}), of
`gates` after mirl_lstm_seq_bwd (H = 512, BWD_BATCHES x T in {1, 5}, with a d_out and with a null one, fed from the saving
forward launch), every number of mirl_lstm_seq_fwd_grid / *_workspace_bytes over GEO_B x GEO_H, and the compute-unit count.
mirl_lstm_seq_status is read once after every launch and must be 0."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "lstm_seq_parent.json")

# (form, H, B); wide (512, 528) has more row blocks than clusters: the clusters loop
FWD_SHAPES = [("narrow", 128, 16), ("narrow", 256, 80), ("narrow", 512, 128), ("wide", 128, 528), ("wide", 256, 272),
              ("wide", 512, 144), ("wide", 512, 528)]
FWD_T = (1, 6)                  # 6 steps re-use both exchange halves with both tag values
BWD_BATCHES = (16, 80, 144, 528)
BWD_T = (1, 5)
GEO_B = (16, 64, 80, 128, 144, 256, 272, 512, 528, 1024)
GEO_H = (128, 256, 512)
# tensor -> (stream, half range); keep is 0 where the stream value is below 0.15
TENSORS = {"gx": (0, 2.0), "w": (1, 0.08), "h0": (2, 3.0), "c0": (3, 1.0), "d_out": (5, 1.0)}
KEEP_STREAM, KEEP_BELOW = 4, 0.15


def unit(stream, n):
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(2654435761) + np.uint64(stream * 40503)) % np.uint64(1 << 32)).astype(np.float64) / float(1 << 32)


def tensor(name, *shape):
    s, a = TENSORS[name]
    return ((2.0 * unit(s, int(np.prod(shape))) - 1.0) * a).astype(np.float32).reshape(shape)


def keep_mask(T, B):
    return (unit(KEEP_STREAM, T * B) >= KEEP_BELOW).astype(np.float32).reshape(T, B)


def lds_of(form, H):
    return (64 * (H + 4) + 4 * 16 * 20) * 4 if form == "wide" else (16 * (H + 4) + 256) * 4


def fwd_key(form, H, B, T, save):
    return "%s-H%d-B%d-T%d-save%d" % (form, H, B, T, save)


def bwd_key(B, T, with_d_out):
    return "B%d-T%d-%s" % (B, T, "d_out" if with_d_out else "null")


def _L():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from rltime_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _status():
    L = _L()
    st = C.c_int32(-1)
    L.check(L.lib.mirl_lstm_seq_status(C.byref(st)), "mirl_lstm_seq_status")
    return st.value


def _workspace(nbytes):
    import torch
    ws = torch.full(((nbytes + 3) // 4,), 3.0, device="cuda")      # finite leftovers with bit 30 set; the launch clears what it must
    assert ws.data_ptr() % 256 == 0
    return ws


def fwd_grid(B, H):
    """-> [workgroups, lds_bytes, compute_units, per_compute_unit]"""
    L = _L()
    wg, lds, cus, per = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
    L.check(L.lib.mirl_lstm_seq_fwd_grid(B, H, C.byref(wg), C.byref(lds), C.byref(cus), C.byref(per)), "mirl_lstm_seq_fwd_grid")
    return [wg.value, lds.value, cus.value, per.value]


def geometry(B, H):
    L = _L()
    need = C.c_int64()
    L.check(L.lib.mirl_lstm_seq_workspace_bytes(B, H, C.byref(need)), "mirl_lstm_seq_workspace_bytes")
    g = {"fwd_grid": fwd_grid(B, H), "workspace_bytes": need.value}
    if H == 512:
        L.check(L.lib.mirl_lstm_seq_bwd_workspace_bytes(B, H, C.byref(need)), "mirl_lstm_seq_bwd_workspace_bytes")
        g["bwd_workspace_bytes"] = need.value
    return g


def run_forward(H, B, T, save):
    """One launch of mirl_lstm_seq_fwd -> (device tensors by name, status).  save: every output; else out and the last state."""
    import torch
    L = _L()
    dev = lambda a: torch.from_numpy(a).cuda()                     # noqa: E731
    new = lambda *s: torch.full(s, float("nan"), device="cuda")    # noqa: E731
    gx, w, h0, c0, keep = dev(tensor("gx", T, B, 4 * H)), dev(tensor("w", 4 * H, H)), dev(tensor("h0", B, H)), dev(tensor("c0", B, H)), dev(keep_mask(T, B))
    r = {"out": new(T, B, H), "h_last": new(B, H), "c_last": new(B, H)}
    if save:
        r.update(gx=gx, c_all=new(T, B, H), hm=new(T + 1, B, H), cm=new(T + 1, B, H))
    need = C.c_int64()
    L.check(L.lib.mirl_lstm_seq_workspace_bytes(B, H, C.byref(need)), "mirl_lstm_seq_workspace_bytes")
    ws = _workspace(need.value)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib.mirl_lstm_seq_fwd(T, B, H, _p(gx), _p(w), _p(h0), _p(c0), _p(keep), _p(r["out"]), _p(r.get("c_all")), _p(r.get("hm")),
                                    _p(r.get("cm")), _p(r["h_last"]), _p(r["c_last"]), int(save), _p(ws), st), "mirl_lstm_seq_fwd")
    torch.cuda.synchronize()
    return r, _status(), (w, keep)


def forward_digests(H, B, T, save):
    r, status, _ = run_forward(H, B, T, save)
    return {k: _digest(v) for k, v in r.items()}, status


def backward_digests(B, T):
    """The saving forward launch at H = 512, then mirl_lstm_seq_bwd with a d_out and with a null one
    -> ({"d_out": digest of gates, "null": digest of gates}, [status after each of the three launches])."""
    import torch
    L = _L()
    H = 512
    fwd, st_f, (w, keep) = run_forward(H, B, T, 1)
    need = C.c_int64()
    L.check(L.lib.mirl_lstm_seq_bwd_workspace_bytes(B, H, C.byref(need)), "mirl_lstm_seq_bwd_workspace_bytes")
    d_out = torch.from_numpy(tensor("d_out", T, B, H)).cuda()
    res, statuses = {}, [st_f]
    for name, dd in (("d_out", d_out), ("null", None)):
        gates = fwd["gx"].clone()
        ws = _workspace(need.value)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(L.lib.mirl_lstm_seq_bwd(T, B, H, _p(gates), _p(w), _p(fwd["c_all"]), _p(fwd["cm"]), _p(dd), _p(keep), _p(ws), st), "mirl_lstm_seq_bwd")
        torch.cuda.synchronize()
        statuses.append(_status())
        res[name] = _digest(gates)
    return res, statuses


def record():
    rec = {"compute_units": fwd_grid(16, 128)[2], "forward": {}, "backward": {}, "geometry": {}}
    for B in GEO_B:
        for H in GEO_H:
            rec["geometry"]["B%d-H%d" % (B, H)] = geometry(B, H)
    for form, H, B in FWD_SHAPES:
        assert fwd_grid(B, H)[1] == lds_of(form, H), "B = %d, H = %d does not launch the %s form here" % (B, H, form)
        for T in FWD_T:
            for save in (0, 1):
                d, status = forward_digests(H, B, T, save)
                assert status == 0, (form, H, B, T, save, status)
                rec["forward"][fwd_key(form, H, B, T, save)] = d
    for B in BWD_BATCHES:
        for T in BWD_T:
            d, statuses = backward_digests(B, T)
            assert statuses == [0, 0, 0], (B, T, statuses)
            for name, dig in d.items():
                rec["backward"][bwd_key(B, T, name == "d_out")] = dig
    return rec


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    rec = record()
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d forward cases, %d backward digests, %d geometry rows, %d compute units"
          % (out, len(rec["forward"]), len(rec["backward"]), len(rec["geometry"]), rec["compute_units"]))
