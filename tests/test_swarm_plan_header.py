"""CPU: include/goldsrl_swarmplan.h (the receding-horizon rule planner of the Swarm env, a planned episode in one call) -- the two
functions it declares are exported by libgoldsrl.so and bound in goldsrl/_ffi_swarmplan.py, the signature dict names exactly the
declared set and shares nothing with the pinned goldsrl.h, and a null handle is refused without a device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_swarmplan
    declared = _declared("goldsrl_swarmplan.h")
    assert declared == {"grl_swarm_plan", "grl_swarm_plan_read"}
    assert set(_ffi_swarmplan.SWARMPLAN_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    assert not declared & _declared("goldsrl_swarmrules.h")
    lib = _ffi.load_library(extra_signatures=_ffi_swarmplan.SWARMPLAN_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_swarmplan.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_swarmplan.h")
    assert callable(_ffi_swarmplan.swarm_plan) and callable(_ffi_swarmplan.swarm_plan_host)


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_swarmplan
    lib = _ffi.load_library(extra_signatures=_ffi_swarmplan.SWARMPLAN_SIGNATURES)
    assert lib.grl_swarm_plan(None, None, None, 1, 1, 1, 1, 0, -1) == _ffi.E_INVALID
    assert lib.grl_swarm_plan_read(None, b"rewards", None, 0) == _ffi.E_INVALID


def test_plan_flags_of_the_scripts():
    import argparse

    import pytest
    from goldsrl.scripts import swarm_rules, train_paac_conv, train_paac_field, train_paac_solow
    assert swarm_rules.plan_arg("8:4") == (8, 4) and swarm_rules.plan_arg("6") == (6, 6) and swarm_rules.plan_arg("4:1") == (4, 1)
    for bad in ("4:5", "0", "3:0", "a", "1:2:3", ""):
        with pytest.raises(argparse.ArgumentTypeError):
            swarm_rules.plan_arg(bad)
    assert swarm_rules.get_arg_parser().parse_args(["--plan", "8:4"]).plan == (8, 4)
    assert swarm_rules.get_arg_parser().parse_args([]).plan is None
    for script in (train_paac_conv, train_paac_field):
        args = script.get_arg_parser().parse_args(["--plan-baseline", "8:4", "--eval-every", "0"])
        assert args.plan_baseline == (8, 4)
        with pytest.raises(SystemExit, match="--plan-baseline plays the eval env"):
            script.main(args)
        assert script.get_arg_parser().parse_args([]).plan_baseline is None
    with pytest.raises(SystemExit):                                          # a Swarm flag: the Solow trainer does not have it
        train_paac_solow.get_arg_parser().parse_args(["--plan-baseline", "8"])


def test_the_planner_refuses_what_the_device_would():
    import pytest
    from goldsrl import _ffi_swarmplan

    class NotSwarm(object):
        kind = -1
    with pytest.raises(ValueError, match="not a Swarm engine"):
        _ffi_swarmplan.swarm_plan(NotSwarm(), [(1, 5, 0, 0, 0, 0)], 2, 1, 4)
    with pytest.raises(ValueError, match="not a Swarm engine"):
        _ffi_swarmplan.swarm_plan_host(NotSwarm(), [(1, 5, 0, 0, 0, 0)], 2, 1, 4)


def test_the_planner_is_exported_by_the_baselines():
    from goldsrl.baselines import DEFAULT_SWARM_RULES, SwarmRulePlanner
    from goldsrl.agents.paac.policy_monitor import DeviceSwarmPolicyMonitor, FieldSwarmPolicyMonitor, SwarmPolicyMonitor
    assert len(DEFAULT_SWARM_RULES) == 20 and callable(SwarmRulePlanner)
    assert DeviceSwarmPolicyMonitor.plan_baseline is SwarmPolicyMonitor.plan_baseline is FieldSwarmPolicyMonitor.plan_baseline
