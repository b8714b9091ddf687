"""CPU: include/goldsrl_tickersearch.h (the cross-entropy search over the six numbers of a Ticker rule, every generation in one
call) -- the two functions it declares are exported by libgoldsrl.so and bound in goldsrl/_ffi_tickersearch.py, the signature dict
names exactly the declared set and shares nothing with the pinned goldsrl.h or the other Ticker headers, a null handle is refused
without a device, and the flags, the baseline class and the monitor's method are where the users expect them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_tickersearch
    declared = _declared("goldsrl_tickersearch.h")
    assert declared == {"grl_ticker_search", "grl_ticker_search_read"}
    assert set(_ffi_tickersearch.TICKERSEARCH_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    for other in ("goldsrl_tickersweep.h", "goldsrl_tickerforesight.h", "goldsrl_gatedeval.h", "goldsrl_swarmsearch.h"):
        assert not declared & _declared(other), other
    lib = _ffi.load_library(extra_signatures=_ffi_tickersearch.TICKERSEARCH_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_tickersearch.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_tickersearch.h")
    for fn in ("ticker_search", "ticker_search_host", "ticker_search_start", "ticker_search_candidates", "ticker_search_refit"):
        assert callable(getattr(_ffi_tickersearch, fn)), fn


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_tickersearch
    lib = _ffi.load_library(extra_signatures=_ffi_tickersearch.TICKERSEARCH_SIGNATURES)
    assert lib.grl_ticker_search(None, None, None, None, None, None, None, 1, 2, 1, 1) == _ffi.E_INVALID
    assert lib.grl_ticker_search_read(None, b"fit", None, 0) == _ffi.E_INVALID


def test_the_search_refuses_a_non_ticker_engine():
    import pytest
    from goldsrl import _ffi_tickersearch
    from goldsrl.baselines import TickerRuleSearch

    class NotTicker(object):
        kind = -1
    for fn in (_ffi_tickersearch.ticker_search, _ffi_tickersearch.ticker_search_host):
        with pytest.raises(ValueError, match="not a Ticker engine"):
            fn(NotTicker(), (1, 0, 0, 1, 0.5, 8), generations=2, candidates=4, elites=2, max_steps=4)
    with pytest.raises(ValueError, match="Ticker env only"):
        TickerRuleSearch(NotTicker())


def test_search_flags_of_the_scripts():
    import argparse

    import pytest
    from goldsrl.scripts import swarm_rules, ticker_search, train_ticker
    accepted = ("8:32:8", "8:32", "8", "2:4:2", "3:4", "1:1024:1024")
    rejected = ("0", "8:1", "8:1025", "8:4:5", "8:4:0", "a", "1:2:3:4", "", "8::2", "-1:4:2")
    table = ["--table", "nowhere.npz"]
    for text in accepted:
        want = swarm_rules.search_arg(text)
        assert ticker_search.get_arg_parser().parse_args(table + ["--search", text]).search == want
        assert train_ticker.get_arg_parser().parse_args(table + ["--search-baseline", text]).search_baseline == want
    for text in rejected:
        with pytest.raises(argparse.ArgumentTypeError):
            swarm_rules.search_arg(text)
        with pytest.raises(SystemExit):
            ticker_search.get_arg_parser().parse_args(table + ["--search=" + text])
        with pytest.raises(SystemExit):
            train_ticker.get_arg_parser().parse_args(table + ["--search-baseline=" + text])
    assert ticker_search.get_arg_parser().parse_args(table).search == (8, 32, 8)
    assert train_ticker.get_arg_parser().parse_args(table).search_baseline is None
    args = ticker_search.get_arg_parser().parse_args(table + ["--envs", "3", "--starts", "all", "--eval-table", "held.npz"])
    assert args.envs == 3 and args.starts == ["all"] and args.eval_table == "held.npz"
    assert ticker_search.starts_arg(["default"]) is None and ticker_search.starts_arg(["all"]).shape == (12, 6)
    assert ticker_search.starts_arg(["1,0,0,1,0.5,8", "0.5,0.5,0.5,0.5,0.05,0"]).tolist() == [[1, 0, 0, 1, 0.5, 8], [0.5, 0.5, 0.5, 0.5, np32(0.05), 0]]
    for bad in (["1,0,0,1,0.5"], ["x"], ["all", "default"]):
        with pytest.raises(ValueError):
            ticker_search.starts_arg(bad)


def np32(v):
    import numpy as np
    return float(np.float32(v))


def test_search_baseline_needs_eval_envs(capsys):
    import pytest
    from goldsrl.scripts import train_ticker
    with pytest.raises(SystemExit):
        train_ticker.parse_args(["--table", "nowhere.npz", "--search-baseline", "2:4:2"])
    assert "--search-baseline plays the eval envs" in capsys.readouterr().err
    args = train_ticker.parse_args(["--table", "nowhere.npz", "--search-baseline", "2:4:2", "--eval-envs", "3"])
    assert args.search_baseline == (2, 4, 2)


def test_the_monitor_and_the_baseline_are_where_users_look():
    from goldsrl.agents.a3c.policy_monitor import GatedPolicyMonitor
    from goldsrl.baselines import TickerRuleSearch
    assert callable(GatedPolicyMonitor.ticker_search_baseline) and callable(GatedPolicyMonitor.write_search_baseline_scalars)
    for name in ("run", "best", "play_on"):
        assert callable(getattr(TickerRuleSearch, name)), name
