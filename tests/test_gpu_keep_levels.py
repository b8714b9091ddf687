"""The gradient step over a rollout at EVERY level of rollout-resident state (csrc/net_train.inc ensure_rollout_bufs, csrc/net_conv.hip
bind_activations / forward_chunk; include/goldsrl_net.h grl_net_keep_info):

  3  conv3 / dense activations, per-env trunk tensors and the 21 index lists come from the rollout's slot
  2  the lists are rebuilt (slot_index, trunk_index, patch_sort); also the top level of GRL_TRUNK_SKIP=off / GRL_NET_EXPAND2=lds
  1  the env-level trunk is evaluated again; the only level of GRL_NET_F_PER_AGENT_TRUNK (another slot layout)
  0  everything is recomputed (GRL_NET_F_RECOMPUTE_FORWARD, or nothing fits)

Which one runs is decided by the device's free memory, so a timed run on a crowded card can land on any of them; small tests always
fit and got level 3.  Here GRL_NET_KEEP_LEVEL / GRL_NET_KEEP_FREE_MB (read when a net is created) select the level, grl_net_keep_info
says which one ran and whether the last gradient step read resident activations, and every level is held to the recomputing form
of the same net: same kernels on the same inputs, in the same order of every sum, so gradient, parameters and statistics are
equal bit for bit at EVERY update (measured on the MI355X before it was asserted: LABNOTES.md section J; the bounds
tests/test_gpu_net.py::test_resident_rollout_activations_equal_recomputation allows after the first update are not needed).
The recomputing form and level 3 are held to the float64 oracle in tests/test_gpu_net_tiles.py (there at all four levels).

Shapes: 10 envs in chunks of 40 samples (40, 40 and a ragged 20: three slots per step) and 20 envs in one chunk per step (the
index side stream of the rollout, side_now).  Every form gets a fresh engine and a fresh net from the same seeds; that the
rollouts are the same (actions, values, y, adv bit for bit) is asserted before any gradient is compared."""
import contextlib
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

PER_AGENT, RECOMPUTE = 1, 2      # GRL_NET_F_PER_AGENT_TRUNK, GRL_NET_F_RECOMPUTE_FORWARD
KNOBS = ("GRL_NET_KEEP_LEVEL", "GRL_NET_KEEP_FREE_MB", "GRL_TRUNK_SKIP", "GRL_NET_EXPAND2", "GRL_NET_GEMM")
CHUNKINGS = {"three_chunks": (10, 40), "one_chunk": (20, 200)}      # name -> (envs, max_chunk_samples)

TWO_UPDATES = (("rollout", 3), ("train", 1e-3), ("rollout", 3), ("train", 1e-3))
UPLOAD = (("rollout", 2), ("scale_params", 1.01), ("train", 1e-3))
SAME_ROLLOUT_TWICE = (("rollout", 2), ("train", 0.0), ("train", 0.0))
T_CHANGES = (("rollout", 3), ("train", 1e-3), ("rollout", 2), ("train", 1e-3), ("rollout", 4), ("train", 1e-3))


@contextlib.contextmanager
def _environ(env):
    """The knobs are read when a net is created: exactly `env` of them is set inside, and the caller's environment comes back."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_PARAMS = []


def _params():
    if not _PARAMS:
        from goldsrl import _ffi_net
        rng = np.random.RandomState(9)
        flat = _ffi_net.glorot_uniform_flat(seed=9)
        at = 0
        for name, shape in _ffi_net.CONV_PARAM_SHAPES:
            n = int(np.prod(shape))
            if name.endswith("_b"):      # the background terms of the shared trunk vanish with zero biases
                flat[at:at + n] = (rng.normal(size=n) * 0.05).astype(np.float32)
            at += n
        flat.setflags(write=False)
        _PARAMS.append(flat)
    return _PARAMS[0]


def _make(chunking, env, flags):
    from goldsrl import _ffi, _ffi_net
    E, chunk = CHUNKINGS[chunking]
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=41)
    eng.reset()
    rng = np.random.RandomState(4)
    for _ in range(3):
        eng.step(O.swarm_transform_actions(rng.normal(size=(E, 10, 2)).astype(np.float32)))
    with _environ(dict(env)):
        net = _ffi_net.ConvNet(eng, max_chunk_samples=chunk, reserved=flags)
    net.set_params(_params())
    return eng, net


def _run(chunking, ops, env=(), flags=0):
    """One form through `ops` on a fresh engine and net: a record per rollout (what it stored) and per gradient step (gradient,
    parameters, statistics, keep_info)."""
    E = CHUNKINGS[chunking][0]
    eng, net = _make(chunking, env, flags)
    before = net.keep_info()
    assert (before["level"], before["slots"], before["resident"]) == (0, 0, False), before      # nothing is chosen before a rollout
    out, T = [], 0
    for op, arg in ops:
        if op == "rollout":
            T = arg
            net.rollout(T, 0)
            eng.wait()
            out.append({"kind": "rollout", "T": T,
                        "actions": net.read_rollout("actions", (T, E * 10, 2)), "values": net.read_rollout("values", (T, E * 10)),
                        "y": net.read_rollout("y", (T, E * 10)), "adv": net.read_rollout("adv", (T, E * 10))})
        elif op == "scale_params":
            net.set_params(net.get_params() * np.float32(arg))
        else:
            st = net.train_rollout(arg)
            out.append({"kind": "train", "T": T, "grads": net.get_grads(), "params": net.get_params(), "stats": st, "info": net.keep_info()})
    net.close()
    eng.close()
    return out


_REF = {}


def _reference(chunking, ops, env=(), flags=0):
    """The recomputing twin of a form (same knobs + GRL_NET_F_RECOMPUTE_FORWARD), evaluated once per module run and never written to."""
    env = tuple(sorted((k, v) for k, v in dict(env).items() if not k.startswith("GRL_NET_KEEP_")))
    key = (chunking, ops, env, flags)
    if key not in _REF:
        ref = _run(chunking, ops, env, flags | RECOMPUTE)
        for r in ref:
            if r["kind"] == "train":
                assert r["info"]["level"] == 0 and r["info"]["slots"] == 0 and not r["info"]["resident"], r["info"]
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _nchunks(chunking):
    E, chunk = CHUNKINGS[chunking]
    return (E + chunk // 10 - 1) // (chunk // 10)


def _where(info):
    return ("keep_info %r -- with less free device memory (%.2f GB seen) than the headroom (%.2f GB) every level falls to 0: a crowded "
            "card, not a wrong level" % (info, info["free_bytes"] / 2.0 ** 30, info["headroom_bytes"] / 2.0 ** 30))


def _compare(got, ref, tag, level=None, resident=None):
    """got against the recomputing form, bit for bit: every rollout (actions, values, y, adv) and every update (gradient,
    parameters, statistics).  level / resident: what keep_info must say at every update."""
    assert [r["kind"] for r in got] == [r["kind"] for r in ref]
    nth, worst = 0, []
    for g, r in zip(got, ref):
        if g["kind"] == "rollout":
            for k in ("actions", "values", "y", "adv"):
                assert np.array_equal(g[k], r[k]), (tag, "rollout before update %d" % nth, k)
            continue
        info = g["info"]
        gs, ps = np.abs(r["grads"]).max(), np.abs(r["params"]).max()
        assert np.isfinite(g["grads"]).all() and gs > 0 and np.abs(g["grads"]).max() > 0, (tag, nth)
        worst.append((np.abs(g["grads"] - r["grads"]).max() / gs, np.abs(g["params"] - r["params"]).max() / ps))
        assert np.array_equal(g["grads"], r["grads"]), (tag, nth, worst)
        assert np.array_equal(g["params"], r["params"]), (tag, nth, worst)
        assert g["stats"] == r["stats"], (tag, nth, g["stats"], r["stats"])
        # the values first: a stale slot shows as a wrong gradient, a level that was not the one asked for as a wrong keep_info
        if level is not None:
            assert info["level"] == level, (tag, nth, _where(info))
        if resident is not None:
            assert info["resident"] == resident[nth], (tag, nth, _where(info))
            if info["resident"]:
                assert info["slots"] >= g["T"] * _nchunks(tag[0]), (tag, nth, info)
        nth += 1
    print("%s: worst |difference| / largest entry per update (gradient, parameters): %s" % (tag, ["%.1e %.1e" % w for w in worst]))


# ---- a. each level equals recomputation

@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("level", [1, 2, 3])
def test_each_level_equals_recomputation_over_two_updates(level, chunking):
    """rollout(3) + update, twice: the second rollout runs on the parameters the first update made, and the slots it reads are the
    refreshed ones."""
    got = _run(chunking, TWO_UPDATES, {"GRL_NET_KEEP_LEVEL": str(level)})
    _compare(got, _reference(chunking, TWO_UPDATES), (chunking, "level", level), level=level, resident=[True, True])


# ---- b. invalidation at every level

@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("level", [1, 2, 3])
def test_a_parameter_upload_invalidates_the_resident_copy(level, chunking):
    got = _run(chunking, UPLOAD, {"GRL_NET_KEEP_LEVEL": str(level)})
    _compare(got, _reference(chunking, UPLOAD), (chunking, "upload at level", level), level=level, resident=[False])


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("level", [1, 2, 3])
def test_a_second_step_on_the_same_rollout_recomputes(level, chunking):
    """lr = 0 leaves the parameters where they are but counts as an update: the first step reads the slots, the second must not --
    and both give the recomputing form's gradient, bit for bit."""
    got = _run(chunking, SAME_ROLLOUT_TWICE, {"GRL_NET_KEEP_LEVEL": str(level)})
    _compare(got, _reference(chunking, SAME_ROLLOUT_TWICE), (chunking, "same rollout twice at level", level), level=level,
             resident=[True, False])
    assert np.array_equal(got[1]["grads"], got[2]["grads"])


# ---- c. T changes between rollouts

@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("level", [1, 2, 3])
def test_rollout_length_changes_between_updates(level, chunking):
    """T = 3, 2, 4: the shorter rollout uses the first slots of the buffer it finds, the longer one needs more than were allocated
    and the buffers are made again (slots >= T x chunks is asserted wherever the step was resident)."""
    got = _run(chunking, T_CHANGES, {"GRL_NET_KEEP_LEVEL": str(level)})
    _compare(got, _reference(chunking, T_CHANGES), (chunking, "T = 3, 2, 4 at level", level), level=level, resident=[True, True, True])
    slots = [g["info"]["slots"] for g in got if g["kind"] == "train"]
    assert slots == [3 * _nchunks(chunking), 3 * _nchunks(chunking), 4 * _nchunks(chunking)], slots


# ---- d. forms that cap the level

CAPPED = {
    "trunk_skip_off": ({"GRL_TRUNK_SKIP": "off"}, 0, 2),
    "expand2_lds": ({"GRL_NET_EXPAND2": "lds"}, 0, 2),
    "per_agent_trunk": ({}, PER_AGENT, 1),
    "gemm_f32_at_level_2": ({"GRL_NET_GEMM": "f32", "GRL_NET_KEEP_LEVEL": "2"}, 0, 2),
}


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("form", sorted(CAPPED))
def test_forms_that_cap_the_level_equal_their_recomputing_twin(form, chunking):
    env, flags, level = CAPPED[form]
    got = _run(chunking, TWO_UPDATES, env, flags)
    _compare(got, _reference(chunking, TWO_UPDATES, env, flags), (chunking, form), level=level, resident=[True, True])
    if flags & PER_AGENT:      # its own slot layout: a3 per agent-sample + the dense stack (d1 d2 p1 v1 v2 + 32 words of sign bits)
        chunk = CHUNKINGS[chunking][1]
        assert got[1]["info"]["slot_bytes"][1] == chunk * (3136 + 2080) * 4, got[1]["info"]


# ---- e. the descent

def test_free_memory_walks_the_levels_down_to_recomputation():
    """GRL_NET_KEEP_FREE_MB just above what each level needs (slots x bytes + headroom, the comparison of ensure_rollout_bufs) gives
    3, 2, 1, and just below the last gives 0.  The variable counts MiB, so T is taken long enough for the levels to lie more than
    2 MiB apart (the index lists of a 40-sample chunk are ~25 KB per slot)."""
    chunking = "three_chunks"
    eng, net = _make(chunking, {}, 0)
    net.rollout(1, 0)
    eng.wait()
    first = net.keep_info()
    net.close()
    eng.close()
    assert first["level"] == 3, _where(first)
    b, headroom, nch = first["slot_bytes"], first["headroom_bytes"], _nchunks(chunking)
    assert headroom == (12 << 30) + CHUNKINGS[chunking][1] * 160000
    T = max(3, -(-(2 << 20) // (nch * min(b[3] - b[2], b[2] - b[1]))))
    assert T <= 64, (T, b)      # a few thousand small launches
    slots = T * nch
    ops = (("rollout", T), ("train", 1e-3))
    ref = _reference(chunking, ops)
    need = {lv: slots * b[lv] + headroom for lv in (1, 2, 3)}
    mib = 1 << 20
    for want, cap_mb in ((3, need[3] // mib + 1), (2, need[2] // mib + 1), (1, need[1] // mib + 1), (0, need[1] // mib)):
        assert want == 3 or cap_mb * mib <= need[want + 1], (want, cap_mb, need)      # the level above does not fit
        got = _run(chunking, ops, {"GRL_NET_KEEP_FREE_MB": str(cap_mb)})
        info = got[1]["info"]
        assert info["free_bytes"] <= cap_mb * mib, info
        assert info["slot_bytes"] == b and info["slots"] == (slots if want else 0), (want, info)
        _compare(got, ref, (chunking, "free MB for level", want), level=want, resident=[want > 0])


# ---- g. bookkeeping of the slot layout (no kernel involved: nothing is rolled out)

@pytest.mark.parametrize("chunk", [40, 200, 330, 500])
def test_slot_sizes_per_level(chunk):
    """bind_activations walks a slot region by region and keep_floats_per_slot sizes it: level 3's list area starts and ends on
    128-byte lines, the levels below stay multiples of 16 bytes (float4 stores), and each level adds something.  This holds the
    SIZES to the layout written out below; that bind_activations' walk ends where such a slot does is checked by
    ensure_rollout_bufs before a slot is written (every rollout of this module would fail with E_INVALID otherwise; LABNOTES.md
    section J has what a slot size that is off by four floats gave)."""
    from goldsrl import _ffi, _ffi_net
    eng = _ffi.Engine(_ffi.ENV_SWARM, 4, seed=41)
    eng.reset()
    for env, flags in (({}, 0), ({"GRL_TRUNK_SKIP": "off"}, 0), ({"GRL_NET_EXPAND2": "lds"}, 0), ({}, PER_AGENT)):
        with _environ(env):
            net = _ffi_net.ConvNet(eng, max_chunk_samples=chunk, reserved=flags)
        info = net.keep_info()
        net.close()
        b = info["slot_bytes"]
        assert (info["level"], info["slots"], info["resident"]) == (0, 0, False), info
        if flags & PER_AGENT:      # one layout only
            assert b[1] == b[2] == b[3] == chunk * (3136 + 2080) * 4 and b[1] % 16 == 0, b
            continue
        assert b[1] % 16 == 0 and b[2] % 16 == 0 and b[3] % 128 == 0, b
        assert 0 < b[1] < b[2] < b[3], b
        # level 1: a3sh per env, d3 + m3 per sample, the dense stack; level 2 adds sraw + a2sh per env, d2s + m2s per sample, ulist
        assert b[1] == 4 * ((chunk // 10) * 3136 + chunk * (1600 + 50 + 2080)), b
        assert b[2] - b[1] == 4 * ((chunk // 10) * (12800 + 5184) + chunk * (576 + 18)) + (chunk * 9 + 15) // 16 * 16, b
    eng.close()


def test_a_free_memory_cap_that_is_no_number_is_refused():
    """GRL_NET_KEEP_FREE_MB read as 0 would quietly give level 0: text that is not decimal digits, or that would overflow the
    conversion to bytes, fails the creation of the net instead."""
    from goldsrl import _ffi, _ffi_net
    eng = _ffi.Engine(_ffi.ENV_SWARM, 4, seed=41)
    eng.reset()
    for text in ("", "lots", "12GB", "-1", " 5", "1e3", str(1 << 44)):
        with _environ({"GRL_NET_KEEP_FREE_MB": text}):
            with pytest.raises(_ffi.GrlError, match="GRL_NET_KEEP_FREE_MB"):
                _ffi_net.ConvNet(eng, max_chunk_samples=40)
    with _environ({"GRL_NET_KEEP_FREE_MB": "0"}):      # a number: nothing fits
        net = _ffi_net.ConvNet(eng, max_chunk_samples=40)
    net.rollout(1, 0)
    eng.wait()
    info = net.keep_info()
    net.close()
    eng.close()
    assert (info["level"], info["slots"], info["free_bytes"]) == (0, 0, 0), info
