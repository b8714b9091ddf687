"""CPU: include/goldsrl_tradesearch.h (the cross-entropy search over the four numbers of a TradeAR1 rule, every generation in one
call) -- the two functions it declares are exported by libgoldsrl.so and bound in goldsrl/_ffi_tradesearch.py, the signature dict
names exactly the declared set and shares nothing with the pinned goldsrl.h or the other TradeAR1 and search headers, a null handle
is refused without a device, and the flag, the script, the baseline class and the monitor's method are where the users expect them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_tradesearch
    declared = _declared("goldsrl_tradesearch.h")
    assert declared == {"grl_trade_search", "grl_trade_search_read"}
    assert set(_ffi_tradesearch.TRADESEARCH_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    for other in ("goldsrl_tradesweep.h", "goldsrl_tradeforesight.h", "goldsrl_tickersearch.h", "goldsrl_swarmsearch.h"):
        assert not declared & _declared(other), other
    lib = _ffi.load_library(extra_signatures=_ffi_tradesearch.TRADESEARCH_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_tradesearch.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_tradesearch.h")
    assert len(_ffi_tradesearch.TRADESEARCH_SIGNATURES["grl_trade_search"][1]) == 12
    for fn in ("trade_search", "trade_search_host", "trade_search_play", "trade_rule4_actions", "trade_search_defaults", "trade_search_start",
               "trade_search_candidates", "trade_search_refit"):
        assert callable(getattr(_ffi_tradesearch, fn)), fn


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_tradesearch
    lib = _ffi.load_library(extra_signatures=_ffi_tradesearch.TRADESEARCH_SIGNATURES)
    assert lib.grl_trade_search(None, None, None, None, None, None, None, None, 1, 2, 1, 1) == _ffi.E_INVALID
    assert lib.grl_trade_search_read(None, b"fit", None, 0) == _ffi.E_INVALID


def test_the_search_refuses_another_engine():
    import pytest
    from goldsrl import _ffi_tradesearch
    from goldsrl.baselines import TradeRuleSearch

    class NotTrade(object):
        kind = -1
    for fn in (_ffi_tradesearch.trade_search, _ffi_tradesearch.trade_search_host):
        with pytest.raises(ValueError, match="not a TradeAR1 engine"):
            fn(NotTrade(), (100, 100, 0, 1), generations=2, candidates=4, elites=2, max_steps=4)
    with pytest.raises(ValueError, match="not a TradeAR1 engine"):
        _ffi_tradesearch.trade_search_play(NotTrade(), (100, 100, 0, 1), 4)
    with pytest.raises(ValueError, match="TradeAR1 env only"):
        TradeRuleSearch(NotTrade())


def test_search_flags_of_the_scripts(capsys):
    import argparse

    import numpy as np
    import pytest
    from goldsrl.scripts import swarm_rules, trade_search, train_trade
    for text in ("8:32:8", "8:32", "8", "2:4:2", "1:1024:1024"):
        want = swarm_rules.search_arg(text)
        assert trade_search.get_arg_parser().parse_args(["--search", text]).search == want
        assert train_trade.get_arg_parser().parse_args(["--search-baseline", text]).search_baseline == want
    for text in ("0", "8:1", "8:1025", "8:4:5", "a", ""):
        with pytest.raises(argparse.ArgumentTypeError):
            swarm_rules.search_arg(text)
        with pytest.raises(SystemExit):
            trade_search.get_arg_parser().parse_args(["--search=" + text])
        with pytest.raises(SystemExit):
            train_trade.get_arg_parser().parse_args(["--search-baseline=" + text])
    args = trade_search.get_arg_parser().parse_args([])
    assert args.search == (8, 32, 8) and (args.n_assets, args.envs, args.steps) == (2, 64, 256) and args.env_seed != args.other_seed
    assert train_trade.get_arg_parser().parse_args([]).search_baseline is None
    assert trade_search.starts_arg(["default"]) is None
    assert trade_search.starts_arg(["100,100,0,1", "220,8.5,-0.87,0.987"]).tolist() == np.array([[100, 100, 0, 1], [220, 8.5, -0.87, 0.987]], np.float32).tolist()
    for bad in (["100,100,0"], ["x"], ["default", "100,100,0,1"], ["1,1,nan,1"]):
        with pytest.raises(ValueError):
            trade_search.starts_arg(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        train_trade.parse_args(["--search-baseline", "2:4:2"])
    assert "--search-baseline plays the eval envs" in capsys.readouterr().err
    assert train_trade.parse_args(["--search-baseline", "2:4:2", "--eval-envs", "3", "--eval-every", "1"]).search_baseline == (2, 4, 2)


def test_the_monitor_and_the_baseline_are_where_users_look():
    from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
    from goldsrl.baselines import TradeRuleSearch
    assert callable(PolicyMonitor.search_baseline) and callable(PolicyMonitor.write_search_baseline_scalars)
    for name in ("run", "best", "play_on"):
        assert callable(getattr(TradeRuleSearch, name)), name
