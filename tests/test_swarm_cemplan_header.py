"""CPU: include/goldsrl_swarmcemplan.h (the search planner of the Swarm env: the rule tuned at every decision, a planned episode in
one call) -- the two functions it declares are exported by libgoldsrl.so and bound in goldsrl/_ffi_swarmcemplan.py, the signature
dict names exactly the declared set and shares nothing with the pinned goldsrl.h or the other Swarm headers, a null handle is refused
without a device, and the flags, the baseline class and the monitors' method are where the users expect them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_swarmcemplan
    declared = _declared("goldsrl_swarmcemplan.h")
    assert declared == {"grl_swarm_cemplan", "grl_swarm_cemplan_read"}
    assert set(_ffi_swarmcemplan.SWARMCEMPLAN_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    for other in ("goldsrl_swarmrules.h", "goldsrl_swarmplan.h", "goldsrl_swarmsearch.h", "goldsrl_replay.h"):
        assert not declared & _declared(other), other
    lib = _ffi.load_library(extra_signatures=_ffi_swarmcemplan.SWARMCEMPLAN_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_swarmcemplan.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_swarmcemplan.h")
    # the declared parameter list is as long as the bound one
    text = re.sub(r"/\*.*?\*/", "", _header("goldsrl_swarmcemplan.h"), flags=re.S)
    params = re.search(r"grl_swarm_cemplan\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(params.split(",")) == len(_ffi_swarmcemplan.SWARMCEMPLAN_SIGNATURES["grl_swarm_cemplan"][1]) == 20
    for fn in ("swarm_cemplan", "swarm_cemplan_host"):
        assert callable(getattr(_ffi_swarmcemplan, fn)), fn


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_swarmcemplan
    lib = _ffi.load_library(extra_signatures=_ffi_swarmcemplan.SWARMCEMPLAN_SIGNATURES)
    assert lib.grl_swarm_cemplan(None, None, None, 0, 0, None, None, None, None, None, None, None, 1, 1, 1, 2, 1, 1, 0, -1) == _ffi.E_INVALID
    assert lib.grl_swarm_cemplan_read(None, b"rewards", None, 0) == _ffi.E_INVALID


def test_the_planner_refuses_a_non_swarm_engine():
    import pytest
    from goldsrl import _ffi_swarmcemplan
    from goldsrl.baselines import SwarmSearchPlanner

    class NotSwarm(object):
        kind = -1
    for fn in (_ffi_swarmcemplan.swarm_cemplan, _ffi_swarmcemplan.swarm_cemplan_host):
        with pytest.raises(ValueError, match="not a Swarm engine"):
            fn(NotSwarm(), None, (1, 5, 0, 0, 0, 1), 2, 1, 1, 4, 2, max_steps=4)
    with pytest.raises(ValueError, match="Swarm env only"):
        SwarmSearchPlanner(NotSwarm())


def test_cem_plan_flags_of_the_scripts():
    import argparse

    import pytest
    from goldsrl.scripts import swarm_rules, train_paac_conv, train_paac_field, train_paac_solow
    arg = swarm_rules.cem_plan_arg
    assert arg("8") == (8, 8, 2, 12, 4) and arg("8:4") == (8, 4, 2, 12, 4) and arg("8:4:3") == (8, 4, 3, 12, 4)
    assert arg("8:4:3:16") == (8, 4, 3, 16, 4) and arg("32:8:2:16:4") == (32, 8, 2, 16, 4) and arg("1:1:1:2:1") == (1, 1, 1, 2, 1)
    assert arg("8:4:1:3") == (8, 4, 1, 3, 3) and arg("8:8:1:1024:1024") == (8, 8, 1, 1024, 1024)
    for bad in ("0", "4:8", "8:0", "8:4:0", "8:4:2:1", "8:4:2:1025", "8:4:2:12:13", "8:4:2:12:0", "a", "1:2:3:4:5:6", "", "8::2", "-1:4"):
        with pytest.raises(argparse.ArgumentTypeError):
            arg(bad)
    assert swarm_rules.get_arg_parser().parse_args(["--cem-plan", "8:4:2:12:4"]).cem_plan == (8, 4, 2, 12, 4)
    assert swarm_rules.get_arg_parser().parse_args([]).cem_plan is None
    for script in (train_paac_conv, train_paac_field):
        args = script.get_arg_parser().parse_args(["--cem-plan-baseline", "8:4", "--eval-every", "0"])
        assert args.cem_plan_baseline == (8, 4, 2, 12, 4)
        with pytest.raises(SystemExit, match="--cem-plan-baseline plays the eval env"):
            script.main(args)
        assert script.get_arg_parser().parse_args([]).cem_plan_baseline is None
    with pytest.raises(SystemExit):                                          # a Swarm flag: the Solow trainer does not have it
        train_paac_solow.get_arg_parser().parse_args(["--cem-plan-baseline", "8"])


def test_the_monitors_share_one_cem_plan_baseline():
    from goldsrl.baselines import SwarmSearchPlanner
    from goldsrl.agents.paac.policy_monitor import DeviceSwarmPolicyMonitor, FieldSwarmPolicyMonitor, SwarmPolicyMonitor
    assert callable(SwarmSearchPlanner)
    assert DeviceSwarmPolicyMonitor.cem_plan_baseline is SwarmPolicyMonitor.cem_plan_baseline is FieldSwarmPolicyMonitor.cem_plan_baseline
