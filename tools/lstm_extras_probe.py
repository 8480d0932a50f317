#!/usr/bin/env python3
"""Time the learner step of the flagship recurrent config WITH the extra-features wrapper (synthetic_atari_iqn_lstm.json +
env_args.extra_features = true, the reference's atari_iqn_lstm.json shape) through bench.py's own timed loop, then print
one JSON line: step time (HIP events at step boundaries), the library's per-kernel rows of the extras kernels and of
k_gemm3_* (mirl_profile_*: calls, ms and algorithmic bytes per step), the device time of the library's own (aten) GEMMs,
and the box's measured copy rate with the two kernels' fraction of it.

    python tools/lstm_extras_probe.py [--steps 30] [--warmup 8] [--replay-size 262144] [--concat]

--concat: the concatenating formulation on this tree (LSTM.split_extras = False, share_online_projection = False).  The
script needs nothing that a tree without csrc/lstm_extras.hip lacks: run there, it times the concatenating learner."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--replay-size", type=int, default=262144)
    ap.add_argument("--concat", action="store_true")
    ap.add_argument("--label", default=None)
    own = ap.parse_args()
    import bench
    sys.argv = ["bench.py", "--gpus", "1", "--steps", str(own.steps), "--warmup", str(own.warmup),
                "--replay-size", str(own.replay_size), "--no-cpu-baseline"]
    args = bench.parse()
    args.profile_steps = 3
    build_config, build_trainer = bench.build_config, bench.build_trainer

    def with_extras(*a, **k):
        config = build_config(*a, **k)
        config.setdefault("env_args", {})["extra_features"] = True
        return config

    seen = {}

    def with_switches(*a, **k):
        trainer = build_trainer(*a, **k)
        for pol in (trainer.policy, trainer.target_policy):
            assert pol.model.extra_input_layer == 1
            seen["X"] = int(pol.model.extra_input_shape[0])
            if own.concat:
                pol.model.layers[1].split_extras = False
        if own.concat:
            trainer.share_online_projection = False
        seen["split"] = bool(getattr(trainer.policy.model.layers[1], "split_extras", False))
        return trainer
    bench.build_config, bench.build_trainer = with_extras, with_switches
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = bench.run_mode(args, "strong", 0, 1, device, None, want_tables=True)
    sm = res["step_ms"]
    rows = {}
    for r in res["table"]:
        if r["name"].startswith("k_lstm_extras") or r["name"].startswith("k_gemm3"):
            n = args.profile_steps
            ms = r["total_ms"] / n
            rows[r["name"]] = {"calls_per_step": r["calls"] / n, "ms_per_step": round(ms, 4),
                               "algorithmic_MB_per_step": round(r["algorithmic_bytes"] / n / 1e6, 2),
                               "GBps": round(r["algorithmic_bytes"] / n / ms / 1e6, 1) if ms > 0 else None}
    from rltime_amd._lib import stream
    peak = bench.copy_peak(device, stream)
    for name in ("k_lstm_extras_add", "k_lstm_extras_wgrad"):
        if name in rows and rows[name]["GBps"]:
            rows[name]["fraction_of_copy_peak"] = round(rows[name]["GBps"] / peak[0], 3)
    lib = res["lib_roof"] or {}
    out = {"label": own.label or ("concat" if own.concat else "split"), "split_extras": seen.get("split"), "X": seen.get("X"),
           "B": res["B"], "T": res["T"], "burn_in": res["P"], "n": res["n"], "replay_size": own.replay_size,
           "steps": own.steps, "warmup": own.warmup,
           "step_ms": {"median": round(float(np.median(sm)), 3), "p10": round(float(np.percentile(sm, 10)), 3),
                       "p90": round(float(np.percentile(sm, 90)), 3), "mean_wall": round(res["dt"] / own.steps * 1e3, 3)},
           "library_contraction_ms_per_step": lib.get("library_contraction_ms"), "aten_device_ms_per_step": lib.get("aten_device_ms"),
           "copy_peak_GBps": round(peak[0], 1), "copy_peak_variant": peak[1], "kernels": rows}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
