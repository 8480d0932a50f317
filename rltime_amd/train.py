"""Host driver: json config -> actors -> trainer (reference rltime/train.py:26-153).

    python -m rltime_amd.train synthetic_atari_iqn_lstm.json --num-envs 64 \
        --conf-update '{"training": {"args": {"total_steps": 200000}}}'

One process per GPU (the reference has no multi-GPU path):

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m rltime_amd.train synthetic_atari_iqn_lstm.json [--scaling strong|weak]

Every rank reads RANK / LOCAL_RANK / WORLD_SIZE, takes its shard of the config
(rltime_amd.parallel.shard_config: envs and replay split by env id; "strong" =
the configured mbatch_size is the global batch), joins the RCCL process group and
trains data-parallel; rank 0 logs.
"""
import argparse
import json
import logging

from rltime_amd.general.config import load_config, validate_config
from rltime_amd.general.loggers import DirectoryLogger, NullLogger
from rltime_amd.general.type_registry import get_registered_type
from rltime_amd.general.utils import deep_dictionary_update


_EXTRA_FEATURES_KEYS = ("include_action", "include_reward", "include_timestep", "clip_reward", "timestep_scale", "use_real_done")


def make_vec_env(env, env_args, num_envs, device, seed=0):
    """env_args["extra_features"] (true: the defaults; a dict: the wrapper's arguments) wraps 'catch' / 'flappy' /
    'synthetic-atari' in acting/extra_features.ExtraFeaturesVecEnv — the reference's env_args.wrappers entry of ExtraFeaturesEnvWrapper."""
    env_args = dict(env_args or {})
    extra = env_args.pop("extra_features", None)
    if extra is None or extra is False:
        return _make_base_vec_env(env, env_args, num_envs, device, seed)
    # (refused before any env is built)
    if isinstance(env, str) and env.startswith("CartPole-"):
        raise ValueError("extra_features: the CartPole envs step on the CPU; the extra-features wrapper is a device kernel "
                         "and wraps 'catch' and 'synthetic-atari' only")
    if env == "MountainCarContinuous-v0":
        raise ValueError("extra_features: the wrapper's one-hot last action needs a Discrete action space; "
                         "'MountainCarContinuous-v0' has a Box one (it wraps 'catch' and 'synthetic-atari' only)")
    if extra is not True and not isinstance(extra, dict):
        raise ValueError("extra_features: true (the wrapper's defaults) or a dict of its arguments %s" % (_EXTRA_FEATURES_KEYS,))
    kwargs = {} if extra is True else dict(extra)
    unknown = set(kwargs) - set(_EXTRA_FEATURES_KEYS)
    if unknown:
        raise ValueError("extra_features: unknown arguments %s (known: %s)" % (sorted(unknown), list(_EXTRA_FEATURES_KEYS)))
    if not any(bool(kwargs.get(k, True)) for k in _EXTRA_FEATURES_KEYS[:3]):
        raise ValueError("extra_features: at least one of include_action / include_reward / include_timestep")
    from rltime_amd.acting.extra_features import ExtraFeaturesVecEnv
    return ExtraFeaturesVecEnv(_make_base_vec_env(env, env_args, num_envs, device, seed), **kwargs)


def _make_base_vec_env(env, env_args, num_envs, device, seed=0):
    if isinstance(env, str) and env.startswith("CartPole-"):
        # the CPU plumbing config (BASELINE configs[0]): the build's own cart-pole, v0 = 200-step episodes, v1 = 500
        limit = (env_args or {}).get("max_episode_steps", 500 if env.endswith("v1") else 200)
        if (env_args or {}).get("device", False):
            # the same cart-pole as ONE HIP kernel per vector step (acting/cartpole_device_env.py): cartpole_dqn / cartpole_iqn
            from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
            return CartPoleDeviceVecEnv(num_envs, max_episode_steps=limit, device=device, seed=seed)
        from rltime_amd.acting.cartpole_env import CartPoleVecEnv
        return CartPoleVecEnv(num_envs, max_episode_steps=limit, seed=seed)
    if env == "MountainCarContinuous-v0":
        # the one Box-action env (the reference's mountaincar_continuous_ppo.json): the build's own car, 999-step episodes
        args = dict(env_args or {})
        unknown = set(args) - {"max_episode_steps", "device"}
        if unknown:
            raise ValueError("MountainCarContinuous-v0: unknown env_args %s" % sorted(unknown))
        limit = args.get("max_episode_steps", 999)
        if args.get("device", False):
            # the same car as ONE HIP kernel per vector step (acting/mountaincar_device_env.py)
            from rltime_amd.acting.mountaincar_device_env import MountainCarDeviceVecEnv
            return MountainCarDeviceVecEnv(num_envs, max_episode_steps=limit, device=device, seed=seed)
        from rltime_amd.acting.mountaincar_env import MountainCarVecEnv
        return MountainCarVecEnv(num_envs, max_episode_steps=limit, seed=seed)
    if env == "catch":
        # the one device-native game (acting/catch_env.py: a single HIP kernel per vector step)
        from rltime_amd.acting.catch_env import CatchVecEnv
        args = dict(env_args or {})
        unknown = set(args) - {"frame_shape", "grid", "n_actions", "visible_rows"}
        if unknown:
            raise ValueError("catch: unknown env_args %s" % sorted(unknown))
        if "frame_shape" in args:
            args["frame_shape"] = tuple(args["frame_shape"])
        return CatchVecEnv(num_envs, device=device, seed=seed, **args)
    if env == "flappy":
        # the long-episode device-native game (acting/flappy_env.py: a single HIP kernel per vector step)
        from rltime_amd.acting.flappy_env import FlappyVecEnv
        args = dict(env_args or {})
        unknown = set(args) - {"frame_shape", "cell", "gap", "spacing", "n_actions", "max_episode_steps", "death_reward", "rgb"}
        if unknown:
            raise ValueError("flappy: unknown env_args %s" % sorted(unknown))
        if "frame_shape" in args:
            args["frame_shape"] = tuple(args["frame_shape"])
        return FlappyVecEnv(num_envs, device=device, seed=seed, **args)
    if env != "synthetic-atari":
        raise ValueError(
            "rltime_amd ships the synthetic vector env ('synthetic-atari'), the device-native games 'catch' and 'flappy', its own "
            "CartPole ('CartPole-v0/-v1') and its own 'MountainCarContinuous-v0': real emulators are CPU code outside the scope of this backend (DESIGN.md)")
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    args = dict(env_args or {})
    args["frame_shape"] = tuple(args.get("frame_shape", (4, 84, 84)))
    return SyntheticAtariVecEnv(num_envs, device=device, seed=seed, **args)


def check_rgb_storage(config):
    """frame_stack_dedup keeps ONE plane per transition and rebuilds the others from earlier transitions; the three planes of
    an rgb Flappy frame are colours of one step, not history: refused before anything is built."""
    history = ((config.get("training") or {}).get("args") or {}).get("history_mode") or {}
    if (config.get("env") == "flappy" and (config.get("env_args") or {}).get("rgb", False)
            and (history.get("args") or {}).get("frame_stack_dedup", False)):
        raise ValueError("frame_stack_dedup: the planes of an rgb flappy frame are one step's colours, not a frame stack "
                         "(env_args.rgb with history_mode.args.frame_stack_dedup)")


def create_actors(config, device="cuda", device_acting=True, use_graph=False):
    """acting/create.py:4-27 for the local synchronous actor."""
    from rltime_amd.acting.actor import Actor
    check_rgb_storage(config)
    acting = config.get("acting", {})
    n = acting.get("actor_envs", 1)
    env = make_vec_env(config.get("env"), config.get("env_args"), n, device)
    if device_acting:
        # the device-resident actor needs a GPU policy and an env that steps on the device; a host env / CPU policy
        # (policy_args.cuda false: the cartpole configs) takes the reference's per-env dict path (actor.py:97-149)
        import torch
        cuda = config.get("policy_args", {}).get("cuda", "auto")
        on_gpu = torch.cuda.is_available() if cuda == "auto" else bool(cuda)
        device_acting = on_gpu and hasattr(env, "step_device")
    # acting.extra_args.fused_step: an actor-critic policy acts on the fused vector step, an MLP DQN / IQN policy on the fused
    # MLP step (other keys stay ignored)
    fused = bool((acting.get("extra_args") or {}).get("fused_step", False))
    return Actor(env, exploration_config=acting.get("exploration"), device=device_acting, use_graph=use_graph,
                 base_env_id=acting.get("env_base", 0), total_env_ids=acting.get("total_envs"), fused_mlp=fused,
                 fused_actor_critic=fused)


def train(config, logger=None, device="cuda", device_acting=True, data_parallel=None, use_graph=False,
          resume=None, on_trainer=None):
    """train.py:26-63.  `data_parallel`: rltime_amd.parallel.DataParallel when this
    process is one rank of a multi-GPU job (config already sharded)."""
    logger = logger or NullLogger(echo=True)
    logger.log_config(config)
    actors = create_actors(config, device, device_acting, use_graph=use_graph)
    training = config["training"]
    trainer_cls = get_registered_type("trainers", training["type"])
    trainer = trainer_cls(logger=logger, actors=actors, model_config=config["model"],
                          policy_args=config.get("policy_args", {}))
    trainer.data_parallel = data_parallel
    # the periodic evaluation (training args eval_episodes) steps envs of its own, keyed apart from the acting envs
    trainer.eval_env_factory = lambda n: make_vec_env(config.get("env"), config.get("env_args"), n, device, seed=1)
    if resume:
        trainer.resume_from = resume
    if on_trainer is not None:
        on_trainer(trainer)
    try:
        trainer.train(**training["args"])
    finally:
        actors.close()
    return trainer


def make_logger(rank, dp, log_dir, log_name=None):
    """Rank 0 writes the log rows; EVERY rank knows the run directory, because full
    checkpoints are one file set per rank (training/resume.py).  create_new()
    uniquifies the name, so rank 0's choice is broadcast."""
    if not log_dir:
        return NullLogger(echo=(rank == 0))
    logger, path = None, None
    if rank == 0:
        logger = DirectoryLogger.create_new(log_dir, log_name)
        path = logger.path
    if dp is not None:
        path = dp.broadcast_object(path)
    return logger if rank == 0 else NullLogger(echo=False, path=path)


def train_from_config(path, num_envs=None, env=None, conf_update=None, log_dir=None, log_name=None,
                      scaling="strong", backend=None, resume=None, seed=None):
    """train.py:66-111, plus the one-process-per-GPU launch."""
    import torch
    from rltime_amd import parallel
    config = load_config(path)
    validate_config(config)
    if env is not None:
        config["env"] = env
    if num_envs is not None:
        config.setdefault("acting", {})["actor_envs"] = num_envs
    if conf_update:
        deep_dictionary_update(config, conf_update)
    rank, world, local, dp = parallel.init_from_env(backend=backend)
    device = "cuda"
    if torch.cuda.is_available():
        torch.cuda.set_device(local % max(torch.cuda.device_count(), 1))
        device = torch.device("cuda", torch.cuda.current_device())
    if dp is not None:
        config = parallel.shard_config(config, rank, world, scaling)
    if seed is not None:
        import random
        import numpy as np
        random.seed(seed + rank); np.random.seed(seed + rank); torch.manual_seed(seed + rank)
    if seed is not None and config["training"]["args"].get("history_mode", {}).get("type") in ("replay", "prioritized_replay"):
        hm = config["training"]["args"]["history_mode"].setdefault("args", {})
        hm.setdefault("seed", seed)          # device-RNG sampling stream (the shard mixes its env_base in)
    logger = make_logger(rank, dp, log_dir, log_name)
    try:
        return train(config, logger, device=device, data_parallel=dp, resume=resume)
    finally:
        if dp is not None:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--num-envs", type=int)
    ap.add_argument("--env")
    ap.add_argument("--log-dir")
    ap.add_argument("--log-name")
    ap.add_argument("--conf-update", type=json.loads)
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="multi-GPU: strong = mbatch_size / envs / replay size are whole-job values split over "
                         "the ranks; weak = every rank keeps the configured values")
    ap.add_argument("--backend", default=None, help="torch.distributed backend (default nccl = RCCL)")
    ap.add_argument("--resume", default=None, help="directory written by a previous run's checkpoints (true resume)")
    ap.add_argument("--seed", type=int, default=None)
    a = ap.parse_args()
    logging.basicConfig(level=logging.INFO)
    train_from_config(a.config, a.num_envs, a.env, a.conf_update, a.log_dir, a.log_name,
                      scaling=a.scaling, backend=a.backend, resume=a.resume, seed=a.seed)


if __name__ == "__main__":
    main()
