"""CPU: include/goldsrl_swarmsearch.h (the cross-entropy search over a Swarm rule's five real numbers, every generation in one
call) -- the two functions it declares are exported by libgoldsrl.so and bound in goldsrl/_ffi_swarmsearch.py, the signature dict
names exactly the declared set and shares nothing with the pinned goldsrl.h or the other Swarm headers, a null handle is refused
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
    from goldsrl import _ffi, _ffi_swarmsearch
    declared = _declared("goldsrl_swarmsearch.h")
    assert declared == {"grl_swarm_search", "grl_swarm_search_read"}
    assert set(_ffi_swarmsearch.SWARMSEARCH_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    for other in ("goldsrl_swarmrules.h", "goldsrl_swarmplan.h", "goldsrl_replay.h"):
        assert not declared & _declared(other), other
    lib = _ffi.load_library(extra_signatures=_ffi_swarmsearch.SWARMSEARCH_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_swarmsearch.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_swarmsearch.h")
    for fn in ("swarm_search", "swarm_search_host", "swarm_search_candidates", "swarm_search_refit"):
        assert callable(getattr(_ffi_swarmsearch, fn)), fn


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_swarmsearch
    lib = _ffi.load_library(extra_signatures=_ffi_swarmsearch.SWARMSEARCH_SIGNATURES)
    assert lib.grl_swarm_search(None, 0, None, None, None, None, None, None, None, 1, 2, 1, 1) == _ffi.E_INVALID
    assert lib.grl_swarm_search_read(None, b"fit", None, 0) == _ffi.E_INVALID


def test_the_search_refuses_a_non_swarm_engine():
    import pytest
    from goldsrl import _ffi_swarmsearch
    from goldsrl.baselines import SwarmRuleSearch

    class NotSwarm(object):
        kind = -1
    for fn in (_ffi_swarmsearch.swarm_search, _ffi_swarmsearch.swarm_search_host):
        with pytest.raises(ValueError, match="not a Swarm engine"):
            fn(NotSwarm(), (1, 5, 0, 0, 0, 1), generations=2, candidates=4, elites=2, max_steps=4)
    with pytest.raises(ValueError, match="Swarm env only"):
        SwarmRuleSearch(NotSwarm())


def test_search_flags_of_the_scripts():
    import argparse

    import pytest
    from goldsrl.scripts import swarm_rules, train_paac_conv, train_paac_field, train_paac_solow
    assert swarm_rules.search_arg("8:32:8") == (8, 32, 8) and swarm_rules.search_arg("8:32") == (8, 32, 8) and swarm_rules.search_arg("8") == (8, 32, 8)
    assert swarm_rules.search_arg("2:4:2") == (2, 4, 2) and swarm_rules.search_arg("3:4") == (3, 4, 4) and swarm_rules.search_arg("1:1024:1024") == (1, 1024, 1024)
    for bad in ("0", "8:1", "8:1025", "8:4:5", "8:4:0", "a", "1:2:3:4", "", "8::2", "-1:4:2"):
        with pytest.raises(argparse.ArgumentTypeError):
            swarm_rules.search_arg(bad)
    assert swarm_rules.get_arg_parser().parse_args(["--search", "2:4:2"]).search == (2, 4, 2)
    assert swarm_rules.get_arg_parser().parse_args([]).search is None
    for script in (train_paac_conv, train_paac_field):
        args = script.get_arg_parser().parse_args(["--search-baseline", "8:32:8", "--eval-every", "0"])
        assert args.search_baseline == (8, 32, 8)
        with pytest.raises(SystemExit, match="--search-baseline plays the eval env"):
            script.main(args)
        assert script.get_arg_parser().parse_args([]).search_baseline is None
    with pytest.raises(SystemExit):                                          # a Swarm flag: the Solow trainer does not have it
        train_paac_solow.get_arg_parser().parse_args(["--search-baseline", "8"])


def test_the_monitors_share_one_search_baseline():
    from goldsrl.baselines import SwarmRuleSearch
    from goldsrl.agents.paac.policy_monitor import DeviceSwarmPolicyMonitor, FieldSwarmPolicyMonitor, SwarmPolicyMonitor
    assert callable(SwarmRuleSearch)
    assert DeviceSwarmPolicyMonitor.search_baseline is SwarmPolicyMonitor.search_baseline is FieldSwarmPolicyMonitor.search_baseline
