"""GPU: the persistent LSTM sweeps (csrc/lstm_seq.hip) write the same bits, and report the same launch geometry, as the commit
before the file's hand-off protocol and host geometry were gathered into helpers.

tests/golden/lstm_seq_parent.json was recorded by tests/golden/record_lstm_seq.py on an MI355X at that commit; this module rebuilds
the same integer-arithmetic inputs, launches through the same C entry points and asserts, with no tolerance and no skip:
  * the SHA-256 of every output of mirl_lstm_seq_fwd (narrow and wide at every H, one and six steps, saving and not) and of `gates`
    after mirl_lstm_seq_bwd (with a d_out and with a null one);
  * every number of mirl_lstm_seq_fwd_grid, mirl_lstm_seq_workspace_bytes and mirl_lstm_seq_bwd_workspace_bytes;
  * through lds_bytes, that every forward case launches the recorded form (a device with another compute-unit count fails here);
  * mirl_lstm_seq_status == 0 after every launch."""
import json

import pytest

from tests.golden import record_lstm_seq as REC

pytestmark = pytest.mark.gpu

with open(REC.FIXTURE) as _f:
    GOLD = json.load(_f)

FWD_CASES = [(form, H, B, T, save) for form, H, B in REC.FWD_SHAPES for T in REC.FWD_T for save in (0, 1)]


def test_the_fixture_holds_every_case_and_this_device_is_the_recorded_one():
    assert sorted(GOLD["forward"]) == sorted(REC.fwd_key(*c) for c in FWD_CASES)
    assert sorted(GOLD["backward"]) == sorted(REC.bwd_key(B, T, d) for B in REC.BWD_BATCHES for T in REC.BWD_T for d in (True, False))
    assert sorted(GOLD["geometry"]) == sorted("B%d-H%d" % (B, H) for B in REC.GEO_B for H in REC.GEO_H)
    for c in FWD_CASES:
        assert sorted(GOLD["forward"][REC.fwd_key(*c)]) == sorted(["out", "h_last", "c_last"] + (["gx", "c_all", "hm", "cm"] if c[4] else []))
    assert REC.fwd_grid(16, 128)[2] == GOLD["compute_units"]


@pytest.mark.parametrize("H", REC.GEO_H)
@pytest.mark.parametrize("B", REC.GEO_B)
def test_launch_geometry_and_workspace_sizes_are_the_parents(B, H):
    assert REC.geometry(B, H) == GOLD["geometry"]["B%d-H%d" % (B, H)]


@pytest.mark.parametrize("form,H,B,T,save", FWD_CASES)
def test_forward_sweep_writes_the_parents_bits(form, H, B, T, save):
    lds = REC.fwd_grid(B, H)[1]
    assert lds == REC.lds_of(form, H), "B = %d, H = %d launches with %d bytes of LDS: not the recorded %s form" % (B, H, lds, form)
    got, status = REC.forward_digests(H, B, T, save)
    assert status == 0, "a workgroup of the sweep gave up waiting (status %d)" % status
    assert got == GOLD["forward"][REC.fwd_key(form, H, B, T, save)]


@pytest.mark.parametrize("T", REC.BWD_T)
@pytest.mark.parametrize("B", REC.BWD_BATCHES)
def test_backward_sweep_writes_the_parents_bits(B, T):
    got, statuses = REC.backward_digests(B, T)
    assert statuses == [0, 0, 0], "a workgroup of a sweep gave up waiting (status after forward, backward, backward: %s)" % statuses
    assert got["d_out"] == GOLD["backward"][REC.bwd_key(B, T, True)]
    assert got["null"] == GOLD["backward"][REC.bwd_key(B, T, False)]
