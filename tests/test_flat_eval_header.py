"""CPU: include/goldsrl_flateval.h (greedy acting and the one-launch evaluation of the flat PAAC policy) -- every function it
declares is exported by libgoldsrl.so and bound in goldsrl/_ffi_flat.py, and goldsrl_flatnet.h brings it along."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"grl_fnet_set_greedy", "grl_fnet_eval", "grl_fnet_read_eval"}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_eval_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_flat
    text = re.sub(r"/\*.*?\*/", "", _header("goldsrl_flateval.h"), flags=re.S)
    declared = set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))
    assert declared == FUNCTIONS
    assert set(_ffi_flat.FNET_EVAL_SIGNATURES) == declared and not declared & set(_ffi_flat.FNET_SIGNATURES)
    lib = _ffi.load_library(extra_signatures=_ffi_flat.FNET_EVAL_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert '#include "goldsrl_flateval.h"' in _header("goldsrl_flatnet.h")
    # the training header's own text still declares none of them (tests/test_cabi_symbols.py reads it against FNET_SIGNATURES)
    flat = re.sub(r"/\*.*?\*/", "", _header("goldsrl_flatnet.h"), flags=re.S)
    assert not FUNCTIONS & set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", flat))
    for method in ("set_greedy", "eval"):
        assert callable(getattr(_ffi_flat.FlatNet, method))


def test_null_net_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_flat
    lib = _ffi.load_library(extra_signatures=_ffi_flat.FNET_EVAL_SIGNATURES)
    assert lib.grl_fnet_set_greedy(None, 1) == _ffi.E_INVALID
    assert lib.grl_fnet_eval(None, 8, 0, 0) == _ffi.E_INVALID
    assert lib.grl_fnet_read_eval(None, b"length", None, 0) == _ffi.E_INVALID


def test_the_learner_and_the_script_know_the_device_monitor():
    from goldsrl.agents.paac import policy_monitor
    from goldsrl.scripts import train_paac_solow
    assert callable(policy_monitor.DeviceSolowPolicyMonitor.eval_once)
    args = train_paac_solow.get_arg_parser().parse_args([])
    assert args.eval_envs == 0 and args.eval_updates == 0 and args.max_episode_steps is None
    args = train_paac_solow.get_arg_parser().parse_args(["--eval-envs", "64", "--eval-updates", "2"])
    assert args.eval_envs == 64 and args.eval_updates == 2
