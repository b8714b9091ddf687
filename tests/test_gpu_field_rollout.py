"""GPU: ConvPolicyVFieldNetwork acting and learning on a Swarm handle (include/goldsrl_fieldrollout.h).

The device's density image against the numpy restatement byte for byte; the once-per-env forward against the float64 oracle and
the per-sample host path; a rollout replayed step by step on a twin engine (the method of tests/test_gpu_conv_rollout_replay.py);
shards; the gradient of a rollout against the oracle, against the per-sample host path and against itself; a clipped Adam step
with its optimizer state carried to a fresh net; the refusals; the learner and the monitor.  Every test that runs a forward runs it
fused (one workgroup per env) and layer by layer (GRL_FIELD_FUSED=off, the parent's arithmetic)."""
import json

import numpy as np
import pytest

import _field_rollout_cases as FC
from oracle import nets as NN

pytestmark = pytest.mark.gpu

PATHS = [pytest.param(True, id="fused"), pytest.param(False, id="layers")]
GEOM_IDS = sorted(FC.GEOMS)
# geometry x path with the reward layout alternating, both layouts on either path
SCENARIOS = [pytest.param(g, f, (i + j) % 2, id="%s-%s-layout%d" % (g, "fused" if f else "layers", (i + j) % 2))
             for i, g in enumerate(GEOM_IDS) for j, f in enumerate((True, False))]
FWD_RTOL, FWD_ATOL, VS_ATOL = 2e-5, 2e-6, 2e-5      # tests/test_gpu_fieldnet.py
GRAD_BOUND = 2e-4


@pytest.mark.parametrize("geom,n_envs", [("G20_L2_F5", 3), ("G20_L2_F5", 70), ("G8_L2_F3", 3), ("G12_L1_F4", 3)])
def test_grid_equals_the_numpy_restatement(geom, n_envs):
    """1. debug_grid on the handle's observations after a reset and after a few steps, an agent and a locust of env 1 outside the box."""
    from goldsrl.agents.state_processors import swarm_field_inputs
    G = FC.GEOMS[geom]["height"]
    eng = FC.engine(geom, n_envs, cap=0)
    n = FC.net(eng, geom)
    rng = np.random.RandomState(4)
    for step in range(4):
        if step == 0:
            FC.share_cells(eng)
        else:
            eng.step(eng.transform_actions(rng.normal(size=(n_envs, 10, 2)).astype(np.float32)))
        lb, ab, ps = eng.read("locust_bins"), eng.read("agent_bins"), eng.read("positions")
        if step == 0:
            assert (lb[1] == 255).any() and (ab[1] == 255).any() and (lb != 255).sum() > 40 * n_envs
        want, _ = swarm_field_inputs(lb, ab, ps, G)
        got = n.debug_grid(lb, ab)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), step
    n.close(); eng.close()


@pytest.mark.parametrize("fused", PATHS)
@pytest.mark.parametrize("geom", GEOM_IDS)
def test_forward_matches_oracle_and_host_predict(geom, fused, monkeypatch):
    """2. predict_swarm against oracle.nets.field_forward in float64 and against FieldNet.predict on the same host samples.  7 envs
    with max_samples = 3: the layer-by-layer path runs chunks of 3, 3 and 1 envs."""
    FC.set_fused(monkeypatch, fused)
    G, L = FC.GEOMS[geom]["height"], FC.GEOMS[geom]["conv_layers"]
    n_envs = 7
    eng = FC.engine(geom, n_envs, cap=0)
    FC.share_cells(eng)
    rng = np.random.RandomState(5)
    for _ in range(2):
        eng.step(eng.transform_actions(rng.normal(size=(n_envs, 10, 2)).astype(np.float32)))
    n, host = FC.net(eng, geom, max_samples=3), FC.net(eng, geom, max_samples=n_envs * 10)
    out = n.predict_swarm()
    states, pos = FC.field_inputs(eng.read("locust_bins"), eng.read("agent_bins"), eng.read("positions"), G)
    mu, sigma, vs = NN.field_forward(FC.params(geom)[0], states.astype(np.float64), pos, FC.SCALE, L)
    ref = host.predict(states, pos)
    for want in ((mu, sigma, vs), (ref["mu"], ref["sigma"], ref["vs"])):
        np.testing.assert_allclose(out["mu"], want[0], rtol=FWD_RTOL, atol=FWD_ATOL)
        np.testing.assert_allclose(out["sigma"], want[1], rtol=FWD_RTOL, atol=FWD_ATOL)
        np.testing.assert_allclose(out["vs"], want[2], rtol=FWD_RTOL, atol=VS_ATOL)
    v = out["vs"].reshape(n_envs, 10)
    assert np.array_equal(v, np.repeat(v[:, :1], 10, axis=1))      # one trunk per env
    assert len(np.unique(v[:, 0])) == n_envs
    n.close(); host.close(); eng.close()


@pytest.mark.parametrize("geom,fused,layout", SCENARIOS)
def test_rollout_replays_on_a_twin(geom, fused, layout, monkeypatch):
    """3. E = 5, T = 4, TimeLimit(3) with staggered counters, action counter from 1000; the twin is stepped with the recorded
    env_actions."""
    sc = FC.scenario(geom, fused, layout, monkeypatch)
    ro, figures = sc["ro"], {}
    assert sc["schedule"].sum() >= FC.E and sc["schedule"].any(axis=1).sum() >= 3      # ends inside the rollout, on different steps
    bad = FC.replay(ro, sc["twin"], sc["tnet"], layout, FC.COUNTER0, sc["schedule"], figures)
    print("worst action error %.3f of its bound (rtol %g, atol %g)" % (figures.get("action_err_of_bound", -1.0), FC.ACT_RTOL, FC.ACT_ATOL))
    assert bad is None, bad
    assert sc["net"].get_action_counter() == FC.COUNTER0 + FC.T == 1004
    y, adv = sc["eng"].returns(ro["rewards"], ro["values"], ro["boot"], FC.GAMMA, scale=FC.SCALE)
    assert np.array_equal(ro["y"], y) and np.array_equal(ro["adv"], adv)
    v = ro["values"].reshape(FC.T, FC.E, 10)
    assert np.array_equal(v, np.repeat(v[:, :, :1], 10, axis=2))


@pytest.mark.parametrize("fused", PATHS)
@pytest.mark.parametrize("geom", GEOM_IDS)
def test_shards_equal_the_whole(geom, fused, monkeypatch):
    """4. one handle of 6 envs against two of 3 at env_id_offset 0 and 3: same seed and parameters, one rollout of 3 steps."""
    FC.set_fused(monkeypatch, fused)
    got = []
    for n_envs, offset in ((6, 0), (3, 0), (3, 3)):
        eng = FC.engine(geom, n_envs, offset=offset, cap=2)
        n = FC.net(eng, geom, counter=7)
        n.rollout(3, 0)
        eng.wait()
        got.append({k: n.read_rollout(k, 3) for k in ("actions", "values", "rewards")})
        n.close(); eng.close()
    whole, a, b = got
    for k in ("actions", "values", "rewards"):
        assert np.array_equal(whole[k][:, :30], a[k]) and np.array_equal(whole[k][:, 30:], b[k]), k
    assert not np.array_equal(a["actions"], b["actions"])


def _check_against(st, grads, want_losses, want_g, shapes, bound, tag):
    np.testing.assert_allclose([st["loss"], st["policy_loss"], st["critic_loss_mean"]], want_losses, rtol=1e-4, atol=1e-6)
    errs = FC.block_errors(grads, want_g, shapes)
    print("%s: largest block error %.3e (%s), bound %.3e" % (tag, max(errs.values()), max(errs, key=errs.get), bound))
    for name, err in errs.items():
        assert err < bound, (tag, name, err)
    np.testing.assert_allclose(st["global_norm"], np.sqrt((NN.flatten_params(want_g, shapes) ** 2).sum()), rtol=1e-4)


@pytest.mark.parametrize("geom,fused,layout", SCENARIOS)
def test_rollout_gradient(geom, fused, layout, monkeypatch):
    """5. train_rollout_grads after the rollout of test 3 (200 agent-samples) against the float64 oracle on the samples rebuilt from
    the recorded observations and actions, against the per-sample host path on the same samples, and against itself."""
    sc = FC.scenario(geom, fused, layout, monkeypatch)
    ro, n = sc["ro"], sc["net"]
    _, shapes, _ = FC.params(geom)
    # three agent-samples of different envs and of different steps on one cell: their head gradients add into the same columns
    cells = (ro["ps"][..., 0].astype(int) * FC.GEOMS[geom]["height"] + ro["ps"][..., 1]).reshape(FC.T, FC.E, 10)
    shared = [c for c in np.unique(cells) if (cells == c).sum() >= 3 and len(np.unique(np.nonzero(cells == c)[1])) >= 3
              and len(np.unique(np.nonzero(cells == c)[0])) >= 2]
    assert shared, "no cell is shared by three envs and two steps"
    st = n.train_rollout_grads()
    grads = n.get_grads()
    losses, g = FC.oracle_grads(ro, geom)
    _check_against(st, grads, losses, g, shapes, GRAD_BOUND, "oracle")
    states, pos, act, adv, y = FC.oracle_samples(ro, geom)
    host = FC.net(sc["eng"], geom, max_samples=states.shape[0])
    hst = host.train(states.astype(np.float32), pos, act, adv, y, lr=0.0, apply_update=False)
    hg = NN.unflatten_params(host.get_grads().astype(np.float64), shapes)
    _check_against(st, grads, [hst["loss"], hst["policy_loss"], hst["critic_loss_mean"]], hg, shapes, GRAD_BOUND, "host path")
    host.close()
    again = n.train_rollout_grads()
    assert np.array_equal(grads, n.get_grads()) and again == st      # fixed-order sums: the same bytes


def test_rollout_gradient_of_1400_samples(monkeypatch):
    """5, larger: E = 70, T = 2 at G = 20 -- 140 env-samples, two slabs of every split sum and 1 400 agent-samples on 400 cells.
    The bound is the existing 2e-4 unless the parent's per-sample path (FieldNet.train, max_samples = 1400) is itself further than
    half of that from the oracle on these samples; then twice its largest block error.
    Measured on MI355X: the parent's path is 3.7e-06 of a block's largest entry from the oracle, the rollout's gradient 1.1e-06
    (pol1_w), so the bound stays at 2e-4."""
    geom, n_envs, steps = "G20_L2_F5", 70, 2
    FC.set_fused(monkeypatch, True)
    _, shapes, _ = FC.params(geom)
    eng = FC.engine(geom, n_envs, cap=0)
    n = FC.net(eng, geom, counter=5)
    n.rollout(steps, 0)
    eng.wait()
    ro = FC.read_rollout(n, steps)
    st = n.train_rollout_grads()
    grads = n.get_grads()
    losses, g = FC.oracle_grads(ro, geom)
    states, pos, act, adv, y = FC.oracle_samples(ro, geom)
    host = FC.net(eng, geom, max_samples=states.shape[0])
    host.train(states.astype(np.float32), pos, act, adv, y, lr=0.0, apply_update=False)
    parent = max(FC.block_errors(host.get_grads(), g, shapes).values())
    bound = max(GRAD_BOUND, 2.0 * parent)
    print("parent's per-sample path: largest block error %.3e against the oracle" % parent)
    _check_against(st, grads, losses, g, shapes, bound, "oracle, 1400 samples")
    n.train_rollout_grads()
    assert np.array_equal(grads, n.get_grads())
    host.close(); n.close(); eng.close()


@pytest.mark.parametrize("fused", PATHS)
def test_update_clip_adam_and_optimizer_state(fused, monkeypatch):
    """6. train_rollout(1e-3) with the clip at half the measured norm against clip_by_global_norm + adam_step of the oracle's
    gradient; the optimizer state set into a fresh net reproduces the next update; the next rollout acts on the new parameters."""
    geom, lr = "G20_L2_F5", 1e-3
    FC.set_fused(monkeypatch, fused)
    p, shapes, flat = FC.params(geom)
    G, L = FC.GEOMS[geom]["height"], FC.GEOMS[geom]["conv_layers"]
    eng1, eng2 = FC.engine(geom), FC.engine(geom)
    n1 = FC.net(eng1, geom, counter=FC.COUNTER0)
    n1.rollout(FC.T, 0)
    eng1.wait()
    ro = FC.read_rollout(n1, FC.T)
    norm = n1.train_rollout_grads()["global_norm"]
    n2 = FC.net(eng2, geom, clip_norm=0.5 * norm, counter=FC.COUNTER0)
    n2.rollout(FC.T, 0)
    eng2.wait()
    assert np.array_equal(n2.read_rollout("actions", FC.T), ro["actions"])      # the same rollout on the second engine
    st = n2.train_rollout(lr)
    np.testing.assert_allclose(st["global_norm"], norm, rtol=1e-6)
    _, g = FC.oracle_grads(ro, geom)
    gf = NN.flatten_params(g, shapes)
    clipped, _ = NN.clip_by_global_norm(gf, 0.5 * norm)
    ref, _, _ = NN.adam_step(flat.astype(np.float64), clipped, np.zeros_like(gf), np.zeros_like(gf), 1, lr)
    new = n2.get_params()
    assert np.abs(new - ref).max() <= 0.05 * lr and not np.array_equal(new, flat)
    # the next rollout acts on the updated parameters: the column-major head copies were refreshed
    opt, counter = n2.get_optimizer_state(), n2.get_action_counter()
    assert opt["adam_step"] == 1 and counter == FC.COUNTER0 + FC.T
    before = n2.predict_swarm()
    states, pos = FC.field_inputs(eng2.read("locust_bins"), eng2.read("agent_bins"), eng2.read("positions"), G)
    mu, _, _ = NN.field_forward(NN.unflatten_params(new.astype(np.float64), shapes), states.astype(np.float64), pos, FC.SCALE, L)
    np.testing.assert_allclose(before["mu"], mu, rtol=FWD_RTOL, atol=FWD_ATOL)
    n2.rollout(FC.T, 0)
    eng2.wait()
    assert np.array_equal(n2.read_rollout("mu", FC.T)[0], before["mu"])
    n2.train_rollout(lr)
    # a fresh net on the first engine (it stands where the second stood after rollout 1) from the read-back state: the same update
    n3 = FC.net(eng1, geom, clip_norm=0.5 * norm, flat=new, counter=counter)
    n3.set_optimizer_state(**opt)
    n3.rollout(FC.T, 0)
    eng1.wait()
    n3.train_rollout(lr)
    assert np.array_equal(n3.get_params(), n2.get_params())
    st3, st2 = n3.get_optimizer_state(), n2.get_optimizer_state()
    assert st3["adam_step"] == st2["adam_step"] == 2 and np.array_equal(st3["adam_m"], st2["adam_m"]) and np.array_equal(st3["adam_v"], st2["adam_v"])
    for x in (n1, n2, n3, eng1, eng2):
        x.close()


def test_refusals():
    """7. by return code, before anything is launched"""
    from goldsrl import _ffi, _ffi_field
    geom = "G8_L2_F3"
    g = FC.GEOMS[geom]

    def refused(eng, code=_ffi.E_INVALID, **kw):
        n = _ffi_field.FieldNet(eng, max_samples=8, **dict(g, **kw))
        for call in (lambda: n.rollout_bind(0.99), n.predict_swarm, lambda: n.rollout(2, 0),
                     lambda: n.debug_grid(np.zeros((1, 80, 2), np.uint8), np.zeros((1, 10, 2), np.uint8))):
            with pytest.raises(_ffi.GrlError) as ei:
                call()
            assert ei.value.code == code, kw
        n.close()

    other = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=1, grid_size=20)
    other.reset()
    refused(other)                          # grid_size 20, height 8
    eng = FC.engine(geom, 2)
    refused(eng, channels=3)
    refused(eng, num_actions=3)
    solow = _ffi.Engine(_ffi.ENV_SOLOW, 2, seed=1)
    solow.reset()
    refused(solow)
    n = FC.net(eng, geom)
    for call, code in ((lambda: n.rollout(0, 0), _ffi.E_INVALID), (lambda: n.rollout(2, 2), _ffi.E_INVALID), (lambda: n.train_rollout(1e-3), _ffi.E_STATE),
                       (n.train_rollout_grads, _ffi.E_STATE), (lambda: n.read_rollout("values", 2), _ffi.E_STATE)):
        with pytest.raises(_ffi.GrlError) as ei:
            call()
        assert ei.value.code == code
    n.rollout(2, 0)
    eng.wait()
    with pytest.raises(_ffi.GrlError) as ei:
        n._check(n.lib.grl_fieldnet_read_rollout(n.n, b"nothing", _ffi._ptr(np.zeros(4, np.float32)), 16))
    assert ei.value.code == _ffi.E_INVALID
    for x in (n, eng, other, solow):
        x.close()


def _learner(tmp_path, argv):
    from goldsrl.agents.paac.emulator_runner import SwarmRunner
    from goldsrl.agents.paac.paac import GridPAACLearner
    from goldsrl.scripts import train_paac_field as S
    args = S.get_arg_parser().parse_args(["-ec", "4", "--max_local_steps", "3", "--eval-every", "0", "--scale", "10", "-lr", "1e-3",
                                          "-df", str(tmp_path / "logs")] + argv)
    nc, ec = S.get_network_and_environment_creator(args)
    return GridPAACLearner(nc, ec, args, SwarmRunner, state_processor=None), args


def test_learner_checkpoint_and_monitor(tmp_path, monkeypatch, capsys):
    """8. GridPAACLearner with the field network: 4 envs x 3 steps, 2 updates; resumed from the checkpoint it runs the third update
    that a net loaded from that checkpoint computes on a fresh engine; the monitor's greedy eval episode replays to its score."""
    from goldsrl import _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvPolicyVFieldNetwork
    from goldsrl.scripts import make_swarm_gif
    FC.set_fused(monkeypatch, True)
    n_envs, steps = 4, 3
    ckpt = str(tmp_path / "ck.npz")
    learner, args = _learner(tmp_path, ["--max_global_steps", str(2 * n_envs * steps), "--checkpoint-every", "2", "--checkpoint-path", ckpt])
    stats = learner.train()
    assert learner.global_step == 2 * n_envs * steps and np.isfinite(list(stats.values())).all()
    net = learner.network.net
    import goldsrl._ffi_field as FF
    init = FF.glorot_uniform_flat(3, **learner.network._geometry())
    assert not np.array_equal(net.get_params(), init) and net.get_optimizer_state()["adam_step"] == 2 and net.get_action_counter() == 2 * steps
    # the monitor: one greedy 128-step episode of Swarm-eval-v0 on a handle of the net's grid size
    mon = PM.FieldSwarmPolicyMonitor(global_policy_net=learner.network, summary_writer=PM.ScalarWriter(str(tmp_path / "eval"), tfevents=False),
                                     learner=learner)
    mon.actions_path = str(tmp_path / "swarm-eval.json")
    total, length, rewards = mon.eval_once()
    assert length == 128 and len(rewards) == 128 and json.load(open(mon.actions_path))["score"] == total
    tags = [json.loads(l)["tag"] for l in open(tmp_path / "eval" / "scalars.jsonl")]
    assert tags == ["eval/total_reward", "eval/episode_length"]
    got, score = make_swarm_gif.main(["--actions", mon.actions_path, "--no-gif"])
    printed = capsys.readouterr().out
    assert "score reproduced" in printed and "score differs" not in printed and got == total == score
    mon.policy_net.net.close(); mon.env._eng.close()
    learner.cleanup()
    # resumed: the third update
    learner2, args2 = _learner(tmp_path, ["--max_global_steps", str(3 * n_envs * steps), "--resume", ckpt])
    learner2.train()
    assert learner2.global_step == 3 * n_envs * steps and learner2.network.net.get_optimizer_state()["adam_step"] == 3
    assert learner2.network.net.get_action_counter() == 3 * steps
    eng = _ffi.Engine(_ffi.ENV_SWARM, n_envs, grid_size=20, seed=1692, max_episode_steps=128, env_id_offset=0)
    eng.reset()
    est = ConvPolicyVFieldNetwork(learner2.network.conf).bind(eng, gamma=args2.gamma)
    est.net.load_checkpoint(ckpt)
    est.net.rollout(steps, 0)
    lr = args2.initial_lr - (3 * n_envs * steps * args2.initial_lr / args2.lr_annealing_steps)
    est.net.train_rollout(lr)
    assert np.array_equal(est.net.get_params(), learner2.network.net.get_params())
    est.net.close(); eng.close()
    learner2.cleanup()
