"""GPU: the fallbacks of the flat net's rollout and gradient step (csrc/net_flat.hip), which no other test makes run.

grl_fnet_rollout takes the persistent kernel (net_flat_rollout.inc) only while (1) the net holds one of the 64 constant-memory
argument slots of the process, (2) the rollout's LDS rows fit a CU (160 KB) and (3) the env count gives at most 512 workgroups of
64; otherwise it takes the graph of launches, and a net without a slot also pairs the fast forward with the general backward in its
gradient step.  Here every rung is made true on purpose -- the slots are used up with filler nets, the rollouts are as long as the
LDS allows and longer, the env count gives two rounds of workgroups and more than 512 -- and the result is held to a twin that
takes the other form bit for bit, and the slotless gradient step to the float64 oracle (oracle/nets.py through _flat_oracle.py).

Which form ran is read off the stage clock (grl_fnet_rollout_stage_times, attached before the first rollout): a persistent launch
clears the stamp count and leaves its own, which depends on T alone (under the true window only the heads' stages stamp: four per
forward); the graph's forward launches add theirs to what is there (none under the true window, whose forward kernel carries no
clock).  So every net's clock is first set going by one predict_env, a GRL_FLAT_ROLLOUT=graph twin that goes through the same
calls says how many stamps a graph rollout adds (_form), and under the true window the second of two chained rollouts is one step
shorter than the first, so that a persistent launch cannot leave the count it found.

The scenarios are those of tests/_flat_cases.py (E = 200: three waves and a partial one; Solow with the staggered TimeLimit,
TradeAR1 with 3 and 16 assets close to depletion), so episodes end inside every rollout on steps that differ from env to env.

Largest gradient block error of the slotless gradient step against the float64 oracle, measured on the MI355X (E = 200, T = 6, the
second of two chained rollouts): Solow 2.4e-5 (sig2_b; bound 1e-3), TradeAR1-3 1.8e-6 (sig3_w; bound 3e-4), TradeAR1-16 5.5e-6
(mu1_b; bound 3e-4); see test_the_slotless_gradient_step_matches_the_oracle."""
import contextlib

import numpy as np
import pytest

import _adam_oracle as AO
import _async_scenarios as SC
import _flat_cases as FC
import _flat_oracle as FO
from _flat_cases import CASES, E, LOSS_SUMS
from oracle import nets as NN
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ALL = sorted(CASES)
GRAD_TOL = {"solow": 1e-3, "trade": 3e-4}      # the rollout path's per-block bounds: GRAD_TOL of tests/test_gpu_flatnet_oracle.py
SLOT_MESSAGE = "no constant-memory argument slot is free for this net"
SLOTS = 64                                     # kFlatArgSlots (net_flat_fast.inc)
CLOCK_CAP = 4096                               # stamps the stage clock holds (fwd_stamp, net_flat_mfma.inc)
STATE = {"solow": ("SOLOW_K", "SOLOW_Z", "SOLOW_E", "SOLOW_TAPE", "SOLOW_TAPE_POS", "NHIST", "ELAPSED", "EPISODE"),
         "trade": ("TRADE_CASH", "TRADE_ASSETS", "TRADE_QUANTITY", "TRADE_PRICES", "NHIST", "ELAPSED", "EPISODE")}


# ------------------------------------------------------------------------------------------ the LDS rule, restated
# rollout_lds_floats (net_flat_rollout.inc) over the forward's rows (net_flat_fast.inc): rows of LS = 65 floats -- FF_ST = 401 rows of
# the forward in front of the S0 rows of the input and one row of window lengths, then three rows (reward, value, mask) per step and
# five rows of per-env ints; rounded up to an even float count; then the float64 account, (2 * n_assets + 2) rows of 64 doubles.
# The true window adds one row of 64 ints behind everything (launch_persistent_rollout).  The launch is given up above 160 KB.
def _lds_floats(case, steps, true_window=False):
    S0 = FC.sizes(case)["static_size"]
    n_assets = CASES[case].get("n", 0)
    off = (401 + S0 + 1 + 3 * steps + 5) * 65
    off += off & 1
    return off + (2 * n_assets + 2) * 64 * 2 + (64 if true_window else 0)


def _fits(case, steps, true_window=False):
    return _lds_floats(case, steps, true_window) * 4 <= 160 * 1024


T_STAR = {"solow": 72, "trade3": 66, "trade16": 41}      # the last step count that fits, from the rule above (asserted below)


# ------------------------------------------------------------------------------------------ helpers
def _rollout(pair, T):
    """One rollout; the stage clock's stamp count before and after it."""
    eng, net = pair
    before = len(net.rollout_stage_times())
    net.rollout(T); eng.wait()
    return before, len(net.rollout_stage_times())


def _form(own, graph):
    """'persistent' or 'graph' from the (before, after) stamp counts of a net and of a GRL_FLAT_ROLLOUT=graph twin that ran the
    same rollout: a graph rollout adds what the twin's added (the clock holds CLOCK_CAP stamps and then stands still; under the
    true window it adds none), the persistent launch starts from zero and stays below the cap.  'unknown' when the twin's clock was
    too full to tell."""
    (b, a), (gb, ga) = own, graph
    assert b > 0 and gb > 0, "the clocks were not set going before the rollout (_pair)"
    if ga < CLOCK_CAP:
        as_graph = min(CLOCK_CAP, b + (ga - gb))
    elif b + (CLOCK_CAP - gb) >= CLOCK_CAP:      # the twin added at least CLOCK_CAP - gb
        as_graph = CLOCK_CAP
    else:
        return "unknown"
    if a == as_graph:
        return "graph"
    assert a < CLOCK_CAP, (own, graph)
    return "persistent"


def _snapshot(pair, case, T, windows=False):
    """Everything a rollout leaves behind: its buffers, the env state, the handle's outputs, the done list, the R6 records, the
    action counter and (last: under the true window it carries the rows forward) the prediction on the current observation."""
    eng, net = pair
    kind = CASES[case]["kind"]
    d = FC.read_rollout(net, T)
    for k in ("y", "adv"):
        d[k] = net.read_rollout(k, (T, eng.E))
    d["boot"] = net.read_rollout("boot", (eng.E,))
    if kind == "solow":
        d["histories"] = net.read_rollout("histories", (T, eng.E, CASES[case]["R"], 2))
    if windows:
        d["windows"] = net.read_windows()
    for f in STATE[kind]:
        d["st_" + f] = eng.get_state(f)
    for o in ("obs", "obs_raw", "reward", "done"):
        d["out_" + o] = eng.read(o)
    d["done_list"] = np.sort(eng.read("done_list")[:int(eng.read("done_count")[0])])
    d["recs"] = np.array([(int(r["step_index"]), int(r["env"]), int(r["length"]), float(r["total_reward"])) for r in eng.episodes_read()])
    d["counter"] = np.array([net.get_action_counter()])
    for k, v in net.predict_env().items():
        d["pred_" + k] = v
    return d


def _assert_same(a, b, label):
    assert sorted(a) == sorted(b), label
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (label, k)


def _pair(case, monkeypatch, true_window=False, **kw):
    """FC.pair with the R6 accounting on and the stage clock attached and set going: the prediction on the reset observation
    stamps it (the worker's window; the true window is switched on behind it)."""
    eng, net = FC.pair(case, monkeypatch, **kw)
    eng.episodes_enable(capacity=8 * eng.E + 16384)      # up to 74 steps of 200 envs close to depletion between two reads
    net.rollout_stage_times()
    net.predict_env()
    assert len(net.rollout_stage_times()) > 0
    if true_window:
        net.set_true_window(True)
    return eng, net


def _chain(pairs, case, T, windows=False, reset_idx=SC.RESET_IDX):
    """Two chained rollouts on every pair, of T steps (windows, i.e. under the true window: T and T - 1, see the module's
    docstring), the host resetting reset_idx in between: per pair the snapshots and the (before, after) clock counts of both."""
    snaps, clocks = [[] for _ in pairs], [[] for _ in pairs]
    for i, steps in enumerate((T, T - 1 if windows else T)):
        for j, pr in enumerate(pairs):
            if i == 1:
                pr[0].reset(reset_idx)
            clocks[j].append(_rollout(pr, steps))
            snaps[j].append(_snapshot(pr, case, steps, windows))
    return snaps, clocks


def _refused(net):
    """The net's evaluation is refused for want of a slot (True) or runs (False)."""
    from goldsrl import _ffi
    try:
        net.eval(1)
    except _ffi.GrlError as e:
        assert e.code == _ffi.E_STATE and SLOT_MESSAGE in str(e), e
        return True
    return False


@contextlib.contextmanager
def _no_free_slot():
    """Uses up the argument slots of the process with one-sample nets on a one-env Solow engine: yields (the fillers that hold a
    slot, in the order they took them -- the last one holds the highest slot, for the slots are handed out lowest first and it took
    the last free one --, the filler that was refused).  Every filler is closed at the end, so that no later test starves."""
    from goldsrl import _ffi, _ffi_flat
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 1, seed=1, rnn_length=5)
    eng.reset()
    fillers = []
    try:
        probe = _ffi_flat.FlatNet(eng, rnn_length=5, max_samples=1)
        leaked = _refused(probe)
        probe.close()
        assert not leaked, "a fresh net gets no argument slot before any filler exists: earlier tests leaked FlatNets, all %d slots are taken" % SLOTS
        for _ in range(SLOTS):
            fillers.append(_ffi_flat.FlatNet(eng, rnn_length=5, max_samples=1))
            if _refused(fillers[-1]):
                break
        else:
            raise AssertionError("%d fillers and every one got a slot: the process has more than %d, or closing a net frees more than its own" % (SLOTS, SLOTS))
        yield fillers[:-1], fillers[-1]
    finally:
        for f in fillers:
            f.close()
        eng.close()


CAP_A = SC.CAP      # section A: T = 6 and a TimeLimit of 9 on staggered counters, about 22 envs end on every step


def _stagger(pairs, case):
    """TradeAR1 as FC.pair leaves Solow: the TimeLimit counters staggered -- and, its window being 20 rows, worker history lengths
    0 .. 25 spread over the envs, so that partial and full windows occur from the first step on (Solow's 5 rows fill by themselves)."""
    if CASES[case]["kind"] == "trade":
        for eng, _ in pairs:
            eng.set_state("ELAPSED", SC.staggered_elapsed(eng.E, CAP_A))
            eng.set_state("NHIST", ((5 * np.arange(eng.E)) % 26).astype(np.int32))


def _assert_dones_and_windows(case, snaps):
    """On the host: episodes ended inside the rollouts, the rows behind a done restart the window, partial and full windows occur."""
    R = CASES[case]["R"]
    masks, nh = np.concatenate([s["masks"] for s in snaps]), np.concatenate([s["nhist"] for s in snaps])
    for s in snaps:
        after = np.zeros(s["masks"].shape, bool)
        after[1:] = s["masks"][:-1] == 0
        assert after.any() and (s["nhist"][after] == 1).all()
    assert (masks == 0).sum() >= E // 4 and sum(len(s["recs"]) for s in snaps) > 0
    assert (nh >= R).any() and ((nh > 1) & (nh < R)).any()


def test_the_lds_rule_gives_the_step_counts_the_tests_sweep():
    for case in ALL:
        assert _fits(case, T_STAR[case]) and not _fits(case, T_STAR[case] + 1), case
    # the true window's extra row: TradeAR1-16 no longer fits at its last step count, the other two still do
    assert {c: _fits(c, T_STAR[c], True) for c in ALL} == {"solow": True, "trade3": True, "trade16": False}
    assert not any(_fits(c, T_STAR[c] + 1, True) for c in ALL)


# ------------------------------------------------------------------------------------------ A. the net without a slot
@pytest.mark.parametrize("true_window", [False, True])
@pytest.mark.parametrize("case", ALL)
def test_a_net_without_an_argument_slot_rolls_out_as_the_graph_of_launches(case, true_window, monkeypatch):
    """The 65th live net of the process: launch_persistent_rollout declines, grl_fnet_rollout takes the graph of launches and
    grl_fnet_eval refuses.  Two chained rollouts (the host resets SC.RESET_IDX in between) against a twin that holds a low slot and
    runs the persistent kernel: every buffer, the prediction, the env state, the action counter and the R6 records bit for bit."""
    T = 6
    pairs = []
    try:
        twin = _pair(case, monkeypatch, true_window, cap=CAP_A); pairs.append(twin)
        graph = _pair(case, monkeypatch, true_window, cap=CAP_A, mode="graph"); pairs.append(graph)
        with _no_free_slot():
            own = _pair(case, monkeypatch, true_window, cap=CAP_A); pairs.insert(0, own)      # GRL_FLAT_ROLLOUT unset: it asks for the persistent form
            _stagger(pairs, case)
            snaps, clocks = _chain(pairs, case, T, windows=true_window)
            for i in range(2):
                _assert_same(snaps[0][i], snaps[1][i], (case, "slotless against the persistent twin", i))
                _assert_same(snaps[2][i], snaps[1][i], (case, "graph twin against the persistent twin", i))
                assert _form(clocks[0][i], clocks[2][i]) == "graph", (case, i, clocks)
                assert _form(clocks[1][i], clocks[2][i]) == "persistent", (case, i, clocks)
            if not true_window:
                _assert_dones_and_windows(case, snaps[0])
            else:
                assert sum((s["masks"] == 0).sum() for s in snaps[0]) >= E // 4
            assert _refused(own[1])
            assert not _refused(twin[1])
    finally:
        FC.close(*pairs)


def _adam_bounds(params, grads, opt, opt1, params1, lr, clip_norm):
    """Section d of test_the_keeping_rollout_and_its_update_match_the_oracle: clip + Adam on the device's own gradient, every
    operation to float32 rounding."""
    step = opt["adam_step"]
    assert opt1["adam_step"] == step + 1
    ref = AO.reference(grads, opt["adam_m"], opt["adam_v"], params, step + 1, lr, clip_norm)
    AO.assert_within(ref, params1, opt1["adam_m"], opt1["adam_v"])
    assert not np.array_equal(params1, params)


@pytest.mark.parametrize("case", ALL)
def test_the_slotless_gradient_step_matches_the_oracle(case, monkeypatch):
    """train_grads_device of a net without a slot: flat_forward_fast_kernel<true> fills the workspace, the general
    flat_backward_kernel reads it -- a pair no other configuration makes.  On the second of two chained slotless rollouts (keep is
    set; the graph form keeps nothing, the step recomputes): the float64 oracle, every block within GRAD_TOL, with one 64-sample
    group left out or counted twice beyond it; a GRL_FLAT_FORWARD=layers net's general forward and backward over the dense windows
    of the same samples; a second pass; one Adam step.  That the fast forward ran is read off the stage clock (the general one
    carries none).
    Measured on the MI355X (E = 200, T = 6, 19 groups of 64 samples, the last of 48), largest block error against the oracle: solow
    2.36e-5 (sig2_b; bound 1e-3), trade3 1.76e-6 (sig3_w; bound 3e-4), trade16 5.52e-6 (mu1_b; bound 3e-4).  The last group left out
    or group 0 counted twice moved some block by 0.17 or more in every case.  Against the layers form the gradients were bitwise
    equal in all three cases, Solow (even D: the forwards are bit-identical) and both TradeAR1 cases."""
    T, lr = 6, 1e-3
    c, sz = CASES[case], FC.sizes(case)
    S0, A, R, N, tol = sz["static_size"], sz["num_actions"], c["R"], T * E, GRAD_TOL[c["kind"]]
    monkeypatch.setenv("GRL_FLAT_FORWARD", "layers")
    layers = FC.pair(case, monkeypatch, cap=CAP_A)      # only its train() on explicit windows is used
    monkeypatch.delenv("GRL_FLAT_FORWARD")
    with _no_free_slot():
        own = _pair(case, monkeypatch, cap=CAP_A)
        one_forward = len(own[1].rollout_stage_times())      # what block 0 of one flat_forward_fast_kernel launch stamps (_pair)
        try:
            _stagger((own,), case)
            own[1].set_keep_activations(True)
            snaps, _ = _chain((own,), case, T)
            ro = snaps[0][1]
            _assert_dones_and_windows(case, snaps[0])
            params = own[1].get_params()
            before = len(own[1].rollout_stage_times())
            stats = own[1].train_rollout_grads()
            assert len(own[1].rollout_stage_times()) == before + one_forward < CLOCK_CAP      # the fast forward, and no fast backward
            grads = own[1].get_grads()
            stats2 = own[1].train_rollout_grads()
            assert grads.tobytes() == own[1].get_grads().tobytes() and stats["global_norm"] == stats2["global_norm"]
            for k in LOSS_SUMS:
                np.testing.assert_allclose(stats2[k], stats[k], rtol=1e-6, atol=0, err_msg=k)
            opt = own[1].get_optimizer_state()
            applied = own[1].apply_grads(lr)
            params1, opt1 = own[1].get_params(), own[1].get_optimizer_state()
            assert _refused(own[1])
            # the general forward and backward on the same samples, their windows written out
            f = lambda k, *s: ro[k].reshape((N,) + s)      # noqa: E731
            win = FO.dense_windows(ro["histories"].reshape(N, R, 2)) if c["kind"] == "solow" else FO.repeated_state_windows(f("states", S0), f("nhist"), R)
            dense = layers[1].train(f("states", S0), win(0, N).astype(np.float32), f("actions", A), f("adv"), f("y"), 0.0, apply_update=False)
            gl = layers[1].get_grads()
        finally:
            FC.close(own, layers)
    assert np.array_equal(params, FC.flat_params(case)) and opt["adam_step"] == 0
    shapes = NN.flat_param_shapes(S0, S0, 32, 32, A)
    p = NN.unflatten_params(params.astype(np.float64), shapes)
    args = (p, f("states", S0), win, f("actions", A), f("adv"), f("y"))
    loss, pl, cl, g, _ = FO.loss_and_grads(*args, 100.0)
    groups = (N + 63) // 64
    sens = FO.sensitivity(g, FO.altered(g, {"group %d left out" % (groups - 1): (-1.0, FO.group_contribution(*args, groups - 1, 100.0)),
                                            "group 0 twice": (1.0, FO.group_contribution(*args, 0, 100.0))}))
    err = FO.block_errors(NN.unflatten_params(grads.astype(np.float64), shapes), g)
    worst = max(err, key=err.get)
    print("\n[slotless] %s: block error %.3g (%s), tolerance %.3g, altered %s, margin %.1fx; against the layers form: max |d| / max %.3g, "
          "bitwise %s" % (case, err[worst], worst, tol, {k: "%.3g (%s)" % v for k, v in sens.items()}, min(e for e, _ in sens.values()) / tol,
                          np.abs(grads - gl).max() / np.abs(gl).max(), grads.tobytes() == gl.tobytes()))
    np.testing.assert_allclose([stats["loss"], stats["policy_loss"], stats["critic_loss_mean"]], [loss, pl, cl], rtol=1e-4, atol=1e-6)
    for label, (e, k) in sens.items():
        assert e > tol, (label, e, k)
    for k, e in err.items():
        assert e < tol, (k, e)
    np.testing.assert_allclose(applied["global_norm"], np.sqrt(sum((v ** 2).sum() for v in g.values())), rtol=1e-4)
    # the layer-by-layer form: the bound of test_fast_forward_form_equals_the_layer_by_layer_form
    np.testing.assert_allclose(grads, gl, rtol=1e-4, atol=1e-6 * np.abs(gl).max() + 1e-9)
    for k in LOSS_SUMS:
        np.testing.assert_allclose(stats[k], dense[k], rtol=1e-4, atol=1e-6, err_msg=k)
    _adam_bounds(params, grads, opt, opt1, params1, lr, own[1].cfg.clip_norm)


@pytest.mark.parametrize("case", ALL)
def test_the_highest_slot_serves_as_the_lowest(case, monkeypatch):
    """The slot the last filler held -- the highest one: they are handed out lowest first -- goes to a new net, which runs the
    persistent kernel, the fast backward from the resident workspace and the evaluation out of g_ro_args / g_flat_args at the far
    end of the arrays, bit for bit as the twin at the front of them."""
    T, lr, cap = 6, 1e-3, CAP_A
    twin = _pair(case, monkeypatch, cap=cap)
    graph = _pair(case, monkeypatch, cap=cap, mode="graph")
    with _no_free_slot() as (holders, _):
        holders[-1].close()
        own = _pair(case, monkeypatch, cap=cap)
        pairs = (own, twin, graph)
        try:
            from goldsrl import _ffi_flat
            again = _ffi_flat.FlatNet(holders[0].eng, rnn_length=5, max_samples=1)      # the freed slot is taken: it was the only one
            assert _refused(again)
            again.close()
            _stagger(pairs, case)
            for _, net in pairs:
                net.set_keep_activations(True)
            snaps, clocks = _chain(pairs, case, T)
            for i in range(2):
                _assert_same(snaps[0][i], snaps[1][i], (case, i))
                assert _form(clocks[0][i], clocks[2][i]) == _form(clocks[1][i], clocks[2][i]) == "persistent", (case, i, clocks)
            # predict_env (in the snapshot) left the resident workspace alone: the gradient step starts at the backward pass
            sa, sb = own[1].train_rollout_grads(), twin[1].train_rollout_grads()
            assert own[1].get_grads().tobytes() == twin[1].get_grads().tobytes() and np.abs(own[1].get_grads()).max() > 0
            ta, tb = own[1].train_rollout(lr), twin[1].train_rollout(lr)
            for x, y in ((sa, sb), (ta, tb)):
                assert x["global_norm"] == y["global_norm"]
                for k in LOSS_SUMS:
                    np.testing.assert_allclose(x[k], y[k], rtol=1e-6, atol=0, err_msg=k)
            assert own[1].get_params().tobytes() == twin[1].get_params().tobytes()
            assert own[1].get_grads().tobytes() == twin[1].get_grads().tobytes()
            oa, ob = own[1].get_optimizer_state(), twin[1].get_optimizer_state()
            assert oa["adam_m"].tobytes() == ob["adam_m"].tobytes() and oa["adam_v"].tobytes() == ob["adam_v"].tobytes()
            assert oa["adam_step"] == ob["adam_step"] == 1
            for tw in (False, True):
                evs = []
                for eng, net in (own, twin):
                    net.set_true_window(tw)
                    eng.reset()
                    eng.set_state("ELAPSED", SC.staggered_elapsed(E, cap))
                    evs.append(net.eval(cap, trace_steps=cap))
                assert (evs[0]["finished"] == 1).all() and len(np.unique(evs[0]["length"])) > 1
                live = np.arange(evs[0]["rewards"].shape[0])[:, None] < evs[0]["length"][None]
                for k in evs[0]:
                    x, y = evs[0][k], evs[1][k]
                    assert x.shape == y.shape, (case, tw, k)
                    if x.ndim >= 2:      # the trace of an env is defined up to its own end
                        x, y = x[live], y[live]
                    assert x.tobytes() == y.tobytes(), (case, tw, k)
        finally:
            FC.close(*pairs)


# ------------------------------------------------------------------------------------------ B. at and past the LDS limit
@pytest.mark.parametrize("group", [None, 64])
@pytest.mark.parametrize("case", ALL)
def test_rollouts_at_and_past_the_lds_limit(case, group, monkeypatch):
    """T* - 1 .. T* + 2 steps (T_STAR): up to T* the persistent kernel, launched at T* with all but a few bytes of the CU's 160 KB
    as dynamic LDS; beyond, the graph of launches.  Two chained rollouts per step count against the GRL_FLAT_ROLLOUT=graph twin,
    with resets, tape refills and depletions inside (the caps lie far below T); at the longest one y and adv against the oracle's
    masked n-step return over that many recorded rows."""
    forms = []
    for T in range(T_STAR[case] - 1, T_STAR[case] + 3):
        own = _pair(case, monkeypatch, group=group, max_samples=T * E)
        graph = _pair(case, monkeypatch, group=group, mode="graph", max_samples=T * E)
        try:
            snaps, clocks = _chain((own, graph), case, T)
        finally:
            FC.close(own, graph)
        for i in range(2):
            _assert_same(snaps[0][i], snaps[1][i], (case, group, T, i))
            assert (snaps[0][i]["masks"] == 0).sum() >= E * (T // CASES[case]["cap"])
        form = [_form(clocks[0][i], clocks[1][i]) for i in range(2)]
        assert form[0] == form[1], (case, T, clocks)
        forms.append(form[0])
    print("\n[lds limit] %s G=%s: T = %d .. %d ran %s" % (case, group, T_STAR[case] - 1, T_STAR[case] + 2, forms))
    assert forms == ["persistent", "persistent", "graph", "graph"], forms      # a prefix of persistent, then graph; both occur
    ro = snaps[0][1]
    oy, oadv = O.nstep_returns(O.rescale_reward(ro["rewards"]).astype(np.float64), ro["values"], ro["boot"], 0.99, ro["masks"].astype(np.float64))
    np.testing.assert_allclose(ro["y"], oy, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ro["adv"], oadv / 100.0, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", ["solow", "trade16"])
def test_a_long_rollout_between_two_short_ones(case, monkeypatch):
    """rollout(20), rollout(T* + 1), rollout(20) on one net that keeps its activations: each against the graph twin; nothing is
    resident behind the long one (the graph keeps nothing), so its gradient step recomputes and equals a keep-off twin's bit for
    bit.  The switch to the graph is sticky today: the third rollout's form is printed, not asserted."""
    long_T = T_STAR[case] + 1
    own = _pair(case, monkeypatch, max_samples=long_T * E)
    graph = _pair(case, monkeypatch, mode="graph", max_samples=long_T * E)
    plain = _pair(case, monkeypatch, max_samples=long_T * E)
    own[1].set_keep_activations(True)
    graph[1].set_keep_activations(True)
    pairs = (own, graph, plain)
    try:
        forms = []
        for i, T in enumerate((20, long_T, 20)):
            clocks = [_rollout(pr, T) for pr in pairs]
            snaps = [_snapshot(pr, case, T) for pr in pairs]
            _assert_same(snaps[0], snaps[1], (case, i, T))
            _assert_same(snaps[2], snaps[1], (case, i, T, "keep off"))
            forms.append(_form(clocks[0], clocks[1]))
            assert _form(clocks[2], clocks[1]) in (forms[-1], "unknown")
            if i == 1:
                sa, sb = own[1].train_rollout_grads(), plain[1].train_rollout_grads()
                assert own[1].get_grads().tobytes() == plain[1].get_grads().tobytes() and np.abs(own[1].get_grads()).max() > 0
                assert sa["global_norm"] == sb["global_norm"]
                for k in LOSS_SUMS:
                    np.testing.assert_allclose(sa[k], sb[k], rtol=1e-6, atol=0, err_msg=k)
        print("\n[lds limit] %s: rollout(20), rollout(%d), rollout(20) ran %s" % (case, long_T, forms))
        assert forms[:2] == ["persistent", "graph"], forms
    finally:
        FC.close(*pairs)


@pytest.mark.parametrize("case", ALL)
def test_the_true_window_at_the_lds_limit(case, monkeypatch):
    """The true window's rollout needs one more row of 64 ints: T* and T* + 1 steps (each followed by a rollout one step shorter)
    against the graph twin, the windows of every sample included; the form is the one the restated rule (_fits) gives --
    TradeAR1-16 at its T* no longer fits."""
    for T in (T_STAR[case], T_STAR[case] + 1):
        own = _pair(case, monkeypatch, True, max_samples=T * E)
        graph = _pair(case, monkeypatch, True, mode="graph", max_samples=T * E)
        try:
            snaps, clocks = _chain((own, graph), case, T, windows=True)
        finally:
            FC.close(own, graph)
        forms = [_form(clocks[0][i], clocks[1][i]) for i in range(2)]
        print("\n[lds limit] %s under the true window: rollout(%d), rollout(%d) ran %s" % (case, T, T - 1, forms))
        for i in range(2):
            _assert_same(snaps[0][i], snaps[1][i], (case, T, i))
        # the second rollout, one step shorter, fits whenever the first did; behind a first one that did not, its form is only printed
        assert forms[0] == ("persistent" if _fits(case, T, True) else "graph") and (forms[1] == "persistent" or forms[0] == "graph"), (case, T, clocks)
        assert snaps[0][1]["nhist"].max() > 1 and (snaps[0][1]["masks"] == 0).sum() >= E * ((T - 1) // CASES[case]["cap"])


# ------------------------------------------------------------------------------------------ C. more workgroups than CUs
@pytest.mark.parametrize("case", ["solow", "trade16"])
def test_a_second_round_of_workgroups(case, monkeypatch):
    """64 * 256 + 37 envs: 257 workgroups of 64 envs (the group size this env count picks), each with a CU's LDS to itself -- the
    last one, of 37 envs, waits for a CU of the first round."""
    n_env, T = 64 * 256 + 37, 4
    own = _pair(case, monkeypatch, n_env=n_env, cap=3, max_samples=T * n_env)
    graph = _pair(case, monkeypatch, n_env=n_env, cap=3, mode="graph", max_samples=T * n_env)
    try:
        snaps, clocks = _chain((own, graph), case, T)
    finally:
        FC.close(own, graph)
    for i in range(2):
        _assert_same(snaps[0][i], snaps[1][i], (case, i))
        assert _form(clocks[0][i], clocks[1][i]) == "persistent", (case, i, clocks)
        assert (snaps[0][i]["masks"] == 0).sum() >= n_env


def test_beyond_512_workgroups_the_default_form_is_the_graph(monkeypatch):
    n_env, T = 64 * 512 + 1, 2
    own = _pair("solow", monkeypatch, n_env=n_env, cap=3, max_samples=T * n_env)
    graph = _pair("solow", monkeypatch, n_env=n_env, cap=3, mode="graph", max_samples=T * n_env)
    try:
        clocks = [_rollout(pr, T) for pr in (own, graph)]
        snaps = [_snapshot(pr, "solow", T) for pr in (own, graph)]
    finally:
        FC.close(own, graph)
    _assert_same(snaps[0], snaps[1], "solow")
    assert _form(clocks[0], clocks[1]) == "graph", clocks
