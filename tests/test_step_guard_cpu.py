"""No GPU: the step guard's surface — the four entry points are exported with argtypes and refuse bad arguments before
anything touches a device, `skip_invalid_steps` travels down the `_train` chain of every Q-learning trainer, and the
set-ups it cannot cover (a CPU policy, an attached process group) are refused with a ValueError that says why."""
import ctypes as C
import inspect

import pytest

GUARDED = ("mirl_step_guard_open", "mirl_adam_clip_step_guarded", "mirl_replay_update_losses_guarded",
           "mirl_lstm_seq_status_device")
GAMMA_ETC = dict(gamma=0.99, nstep_train=1, lr=1e-3)


def test_entry_points_are_exported_with_argtypes():
    from rltime_amd import _lib
    for name in GUARDED:
        assert name in _lib._SIGNATURES, name
        fn = getattr(_lib.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(_lib._SIGNATURES[name]) and fn.restype is C.c_int
    plain, guarded = _lib._SIGNATURES["mirl_adam_clip_step"], _lib._SIGNATURES["mirl_adam_clip_step_guarded"]
    assert guarded[:len(plain) - 1] == plain[:-1] and len(guarded) == len(plain) + 1          # the same arguments + the guard
    plain, guarded = _lib._SIGNATURES["mirl_replay_update_losses"], _lib._SIGNATURES["mirl_replay_update_losses_guarded"]
    assert len(guarded) == len(plain) + 1


def test_header_declares_the_four_prototypes_and_the_veto_bits():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mirl.h")).read()
    for name in GUARDED:
        assert "int %s(" % name in text, name
    for line in ("#define MIRL_VETO_LOSS 1", "#define MIRL_VETO_NORM 2", "#define MIRL_VETO_STATUS 4"):
        assert line in text
    from rltime_amd.models.torch import optim
    assert (optim.VETO_LOSS, optim.VETO_NORM, optim.VETO_STATUS, optim.GUARD_WORDS) == (1, 2, 4, 8)


def test_bad_arguments_are_refused_on_the_host():
    """MIRL_ERR_ARG before any launch: callable without a device."""
    from rltime_amd import _lib
    lib = _lib.lib
    word = (C.c_int32 * 12)()
    base = C.addressof(word)
    aligned = base + (-base) % 16
    assert lib.mirl_step_guard_open(None, None, 0, None, 0, None) == _lib.MIRL_ERR_ARG
    assert "guard" in _lib.last_error()
    assert lib.mirl_step_guard_open(C.c_void_p(aligned + 4), None, 0, None, 0, None) == _lib.MIRL_ERR_ARG
    assert lib.mirl_step_guard_open(C.c_void_p(aligned), None, -1, None, 0, None) == _lib.MIRL_ERR_ARG
    assert lib.mirl_step_guard_open(C.c_void_p(aligned), None, 3, None, 0, None) == _lib.MIRL_ERR_ARG
    assert lib.mirl_step_guard_open(C.c_void_p(aligned), None, 0, None, 5, None) == _lib.MIRL_ERR_ARG
    assert lib.mirl_step_guard_open(C.c_void_p(aligned), None, 0, None, 1, None) == _lib.MIRL_ERR_ARG
    assert lib.mirl_adam_clip_step_guarded(1, None, None, None, None, None, None, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, None, 0,
                                           None, None, None) == _lib.MIRL_ERR_ARG
    assert lib.mirl_replay_update_losses_guarded(None, 1, None, None, None, None) == _lib.MIRL_ERR_ARG
    assert lib.mirl_lstm_seq_status_device(None) == _lib.MIRL_ERR_ARG
    assert list(word) == [0] * 12


def test_python_surface_takes_the_guard():
    from rltime_amd.models.torch.optim import ClipAdam
    from rltime_amd.history.replay_history import ReplayHistoryBuffer, PrioritizedReplayHistoryBuffer
    for fn in (ClipAdam.step_clipped, ReplayHistoryBuffer.update_losses, PrioritizedReplayHistoryBuffer.update_losses):
        p = inspect.signature(fn).parameters["guard"]
        assert p.default is None
    # update_losses stays a no-op for non-prioritized buffers, with or without a guard
    assert ReplayHistoryBuffer.update_losses(object(), None, None, guard=object()) is None


class _Policy:
    def __init__(self, cuda):
        self._cuda = cuda

    def is_cuda(self):
        return self._cuda


class _Group:
    active = True


def _trainer(name, cuda, group):
    from rltime_amd.general.type_registry import get_registered_type
    import rltime_amd.training  # noqa: F401  (registers the trainers)
    cls = get_registered_type("trainers", name)
    tr = cls.__new__(cls)
    tr.policy, tr.data_parallel, tr.clip_rewards = _Policy(cuda), group, True
    return tr


@pytest.mark.parametrize("name", ["dqn", "iqn", "dist_dqn"])
def test_option_is_accepted_by_every_q_trainer_and_refused_for_a_cpu_policy(name):
    """A TypeError would mean the keyword does not travel down the `_train` chain; what comes back instead is TorchTrainer's
    own refusal of a CPU policy, raised before anything is allocated."""
    tr = _trainer(name, cuda=False, group=None)
    with pytest.raises(ValueError, match="CPU policy"):
        tr._train(skip_invalid_steps=True, **GAMMA_ETC)


@pytest.mark.parametrize("name", ["dqn", "iqn", "dist_dqn"])
def test_option_is_refused_under_a_process_group(name):
    tr = _trainer(name, cuda=True, group=_Group())
    with pytest.raises(ValueError, match="process group"):
        tr._train(skip_invalid_steps=True, **GAMMA_ETC)


def test_dynamic_clip_is_refused_before_anything_is_allocated():
    tr = _trainer("dqn", cuda=True, group=None)
    with pytest.raises(ValueError, match="clip_grad_dynamic_alpha"):
        tr._train(skip_invalid_steps=True, clip_grad=10.0, clip_grad_dynamic_alpha=0.99, **GAMMA_ETC)


def test_option_is_off_by_default_and_optional():
    from rltime_amd.training.torch_trainer import TorchTrainer
    p = inspect.signature(TorchTrainer._train).parameters["skip_invalid_steps"]
    assert p.default is False


def test_signature_pin_still_passes():
    from tests import test_abi
    test_abi.test_mirror_classes_keep_the_reference_signatures()
