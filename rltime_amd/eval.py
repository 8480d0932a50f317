"""Entry point for evaluating a trained policy (reference rltime/eval.py, built without rendering and recording:
DESIGN.md section 7).

    python -m rltime_amd.eval <run directory> --num-envs 32 --episodes 1000 --eps 0.001

Loads config.json and checkpoint.p of a run directory written by `python -m rltime_amd.train ... --log-dir`, acts with a
fixed small epsilon on `num_envs` device envs and reports reward / length statistics of the first `episodes` episodes
that STARTED (eval.py:59-72), appended as one line to eval.json.  The acting and the counting run as one captured
rollout graph on the GPU (acting/evaluator.py, csrc/acting.hip k_eval_count).  With eps > 0 the random actions come from
the device actor's Philox stream keyed by `seed`, not from np.random like the reference's: only eps = 0 is comparable
with the reference run for run."""
import argparse
import datetime
import time

from rltime_amd.general.config import load_config
from rltime_amd.general.loggers import DirectoryLogger
from rltime_amd.general.type_registry import get_registered_type


def create_policy_from_config(config, action_space, observation_space):
    """eval.py:16-34: the policy of the config's trainer class; the weights are not loaded."""
    if not isinstance(config, dict):
        config = load_config(config)
    train_cls = get_registered_type("trainers", config["training"].get("type", None))
    if not hasattr(train_cls, "create_policy"):
        raise ValueError("config training class %s has no create_policy" % train_cls)
    return train_cls.create_policy(model_config=config.get("model"), action_space=action_space,
                                   observation_space=observation_space, **config.get("policy_args", {}))


def _plain(stats, integral):
    """numpy scalars -> what json writes as numbers."""
    return {k: (int(v) if integral and k in ("min", "max") else float(v)) for k, v in stats.items()}


def make_record(step, evaluator_record, seconds):
    """The reference's result (eval.py:164-178) plus `steps` (vector steps consumed) and `seconds`."""
    r = evaluator_record
    return {"step": step, "date": datetime.datetime.now(), "episodes": r["episodes"], "envs": r["envs"],
            "reward": _plain(r["reward"], False), "length": _plain(r["length"], True), "steps": int(r["steps"]),
            "seconds": float(seconds)}


def eval_policy(path, num_envs, episode_count, record=False, record_fps=60, render=False, render_fps=None, eps=0.001,
                seed=0):
    """eval.py:37-180.  `seed` keys the env and the actor's draws.  Returns the record it appends to <path>/eval.json."""
    if record or render:
        raise ValueError("rltime_amd.eval is built without rendering and recording (DESIGN.md section 7): "
                         "record / render must stay False")
    if num_envs > episode_count:
        raise ValueError("num_envs can't be higher than the requested episode_count")
    import torch
    from rltime_amd.acting.evaluator import Evaluator
    from rltime_amd.train import make_vec_env
    logger = DirectoryLogger(path, echo=False)
    config = logger.get_config()
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
    env = make_vec_env(config.get("env"), config.get("env_args"), num_envs, device, seed=seed)
    try:
        policy = create_policy_from_config(config, env.action_space, env.observation_space)
        training_step, cp_data = logger.get_checkpoint()
        policy.load_state(cp_data["policy_state"])
        t0 = time.time()
        # the run's own opt-in (acting.extra_args.fused_step): an MLP policy on float32 observations evaluates on the fused MLP step
        fused = bool(((config.get("acting") or {}).get("extra_args") or {}).get("fused_step", False))
        got = Evaluator(policy, env, episode_count, eps=eps, seed=seed, fused_mlp=fused).run()
        result = make_record(training_step, got, time.time() - t0)
    finally:
        env.close()
    logger.log_result("eval", result, None)
    return result


def main():
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("path", help="the training run directory to evaluate")
    ap.add_argument("--num-envs", type=int, default=1, help="envs to run in parallel")
    ap.add_argument("--episodes", type=int, default=5, help="episodes to evaluate")
    ap.add_argument("--eps", type=float, default=0.001, help="epsilon of the random action selection")
    ap.add_argument("--seed", type=int, default=0, help="keys the env and the actor's draws")
    a = ap.parse_args()
    result = eval_policy(a.path, num_envs=a.num_envs, episode_count=a.episodes, eps=a.eps, seed=a.seed)
    for key in sorted(result):
        print("  %s: %s" % (key, result[key]))


if __name__ == "__main__":
    main()
