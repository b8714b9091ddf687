"""The observation index record (obs_index_kernel, csrc/net_shared.inc) and the backward helpers that read it.

GRL_OBS_INDEX=off selects the kernels that derive the bins' buckets and the agents' pixel tables inside the full-grid kernels; the
default reads them from a record a small kernel writes once per forward and once per backward chunk pass (the forward's conv1
reads its touched pixels and its windows' taps from it).  Both are the same sums in the same order, so
heads and the whole flat gradient must be EQUAL bit for bit.  The record itself is restated in plain numpy below (from its written
layout, not from the kernel's way of computing it); the restatement is checked against independent formulations without a GPU, and
the device's record against the restatement word for word."""
import numpy as np
import pytest

WORDS, OFF, LIST, PIX, CSLOT, SLOTPIX, PM, LIST2 = 288, 4, 16, 112, 152, 162, 182, 196
G = 84
STATES = ("reset", "interior", "one_bin", "all_outside", "one_tap_class", "two_agents_one_pixel", "agent_on_locust_bin")


# ------------------------------------------------------------------------------------------ the record in numpy
def record_numpy(lb, ab, pos):
    """(288,) uint32 record of one env: lb (80, 2), ab (10, 2), pos (10, 2) uint8; 255 in column 0 = outside the box."""
    rec = np.zeros(WORDS, np.uint32)
    by = rec.view(np.uint8)                      # little-endian bytes of the words
    bins = {}                                    # (channel, h, w) -> [count, lowest point id]
    for pid in range(90):
        c, (h, w) = (0, lb[pid]) if pid < 80 else (1, ab[pid - 80])
        if h == 255:
            continue
        e = bins.setdefault((c, int(h), int(w)), [0, pid])
        e[0] += 1
    first = sorted(bins.items(), key=lambda kv: (kv[0][0], (kv[0][1] % 4) * 4 + kv[0][2] % 4, kv[1][1]))
    for i, ((c, h, w), (k, _)) in enumerate(first):
        rec[LIST + i] = h | (w << 8) | (c << 16) | (k << 20)
    bucket = [c * 16 + (h % 4) * 4 + w % 4 for (c, h, w), _ in first]
    for b in range(33):
        by[OFF * 4 + b] = sum(1 for x in bucket if x < b)
    second = sorted(bins.items(), key=lambda kv: (kv[0][1], kv[0][0], kv[0][2]))      # (h, channel, w)
    for i, ((c, h, w), (k, _)) in enumerate(second):
        rec[LIST2 + i] = h | (w << 8) | (c << 16) | (k << 20)
    for (c, h, w) in bins:                       # touched pixels: the four conv1 outputs whose 8 x 8 / stride 4 window holds the bin
        for dy in (0, 1):
            for dx in (0, 1):
                oy, ox = h // 4 - dy, w // 4 - dx
                if 0 <= oy < 20 and 0 <= ox < 20:
                    p = oy * 20 + ox
                    rec[PM + p // 32] |= np.uint32(1 << (p % 32))
    slots = []
    half = rec.view(np.uint16)
    for cand in range(40):                       # (agent, cover) candidates of the agents' own positions
        a, cov = cand // 4, cand % 4
        ph, pw = int(pos[a][0]), int(pos[a][1])
        oy, ox = ph // 4 - cov // 2, pw // 4 - cov % 2
        if 0 <= oy < 20 and 0 <= ox < 20:
            p, tap = oy * 20 + ox, (ph - 4 * oy) * 8 + (pw - 4 * ox)
            rec[PIX + cand] = p | (tap << 16)
            if p not in slots:
                slots.append(p)
            by[CSLOT * 4 + cand] = slots.index(p)
        else:
            rec[PIX + cand] = 0xFFFFFFFF
            by[CSLOT * 4 + cand] = 255
    for s, p in enumerate(slots):
        half[SLOTPIX * 2 + s] = p
    n0 = sum(1 for (c, _, _) in bins if c == 0)
    rec[0] = n0 | (len(bins) << 8) | (len(slots) << 16)
    return rec


def records_numpy(lb, ab, pos):
    return np.stack([record_numpy(lb[e], ab[e], pos[e]) for e in range(len(lb))])


# ------------------------------------------------------------------------------------------ states
def crafted(state, rng):
    """One env's (lb, ab, pos) of a crafted state."""
    lb = rng.randint(0, G, size=(80, 2)).astype(np.uint8)
    pos = rng.randint(0, G, size=(10, 2)).astype(np.uint8)
    ab = pos.copy()
    if state == "one_bin":                       # all 80 locusts in one bin: one list entry of count 80
        lb[:] = (rng.randint(0, G), rng.randint(0, G))
    elif state == "all_outside":                 # every point outside the box: empty lists; positions are clamped to the rim (digitize)
        lb[:, 0] = 255
        ab[:, 0] = 255
        pos[:] = rng.choice([0, G - 1], size=(10, 2))
    elif state == "one_tap_class":               # every bin of one q = (h % 4, w % 4): one bucket per channel holds everything
        qh, qw = rng.randint(0, 4), rng.randint(0, 4)
        lb[:, 0] = rng.randint(0, 21, size=80) * 4 + qh
        lb[:, 1] = rng.randint(0, 21, size=80) * 4 + qw
        pos[:, 0] = rng.randint(0, 21, size=10) * 4 + qh
        pos[:, 1] = rng.randint(0, 21, size=10) * 4 + qw
        ab = pos.copy()
    elif state == "two_agents_one_pixel":        # agents 2 and 7 in one bin, 3 and 4 in one conv1 pixel but different bins
        pos[7] = pos[2]
        pos[3] = (40, 44)
        pos[4] = (41, 46)
        ab = pos.copy()
    elif state == "agent_on_locust_bin":         # the two count channels meet in one bin (distinct list entries), one agent outside
        pos[0] = lb[5]
        pos[9] = lb[79]
        ab = pos.copy()
        ab[4, 0] = 255
    else:
        raise ValueError(state)
    return lb, ab, pos


def engine_obs(eng):
    eng.observe()
    eng.wait()
    return eng.read("locust_bins"), eng.read("agent_bins"), eng.read("positions")


def interior_obs(eng, rng):
    """Agents moved into the interior of the observation box, as bench.py's interior leg does."""
    x = eng.get_state("SWARM_X")
    E = x.shape[0]
    xa = np.empty((E, 10, 2))
    xa[:, :, 0] = x[:, :, 0].mean(axis=1)[:, None] + rng.uniform(-1.2, 0.0, size=(E, 10))
    xa[:, :, 1] = rng.uniform(1.5, 4.3, size=(E, 10))
    eng.set_state("SWARM_XA", xa)
    return engine_obs(eng)


def mixed_obs(eng, E, states, seed):
    """E envs cycling through `states`; the engine supplies its own reset states and the interior ones."""
    rng = np.random.RandomState(seed)
    eng.reset()
    rl, ra, rp = [a.copy() for a in engine_obs(eng)]
    il, ia, ip = [a.copy() for a in interior_obs(eng, rng)]
    lb, ab, pos = np.empty((E, 80, 2), np.uint8), np.empty((E, 10, 2), np.uint8), np.empty((E, 10, 2), np.uint8)
    for e in range(E):
        s = states[e % len(states)]
        lb[e], ab[e], pos[e] = (rl[e], ra[e], rp[e]) if s == "reset" else (il[e], ia[e], ip[e]) if s == "interior" else crafted(s, rng)
    return lb, ab, pos


def crafted_batch(E, seed):
    rng = np.random.RandomState(seed)
    cr = [s for s in STATES if s not in ("reset", "interior")]
    obs = [crafted(cr[e % len(cr)], rng) for e in range(E)]
    return tuple(np.stack([o[i] for o in obs]) for i in range(3))


# ------------------------------------------------------------------------------------------ without a GPU: the restatement
def test_record_restatement_against_independent_formulations():
    lb, ab, pos = crafted_batch(60, seed=4)
    rng = np.random.RandomState(9)
    lb[50:, :, :] = rng.randint(30, 40, size=(10, 80, 2))          # crowded: many shared bins
    lb[55:, ::3, 0] = 255
    recs = records_numpy(lb, ab, pos)
    for e in range(len(lb)):
        rec, by, half = recs[e], recs[e].view(np.uint8), recs[e].view(np.uint16)
        n0, n, nslots = int(rec[0] & 255), int((rec[0] >> 8) & 255), int(rec[0] >> 16)
        ent = [(int(w >> 16) & 15, int(w) & 255, int(w >> 8) & 255, int(w >> 20)) for w in rec[LIST:LIST + n]]      # (c, h, w, count)
        # dense count grids (what the reference's histogram is) hold exactly the listed bins with the listed counts
        grid = np.zeros((2, G, G), int)
        for c, arr in ((0, lb[e]), (1, ab[e])):
            for h, w in arr:
                if h != 255:
                    grid[c, h, w] += 1
        assert len(set(x[:3] for x in ent)) == n == int((grid > 0).sum()) and n0 == int((grid[0] > 0).sum())
        assert all(grid[c, h, w] == k for c, h, w, k in ent)
        assert not rec[LIST + n:PIX].any()
        # first order: buckets (channel, q) ascending with the offsets as their boundaries; inside a bucket by lowest point id
        off = by[OFF * 4:OFF * 4 + 33].astype(int)
        assert off[0] == 0 and off[16] == n0 and off[32] == n and (np.diff(off) >= 0).all()
        pts = [(0, int(h), int(w)) for h, w in lb[e]] + [(1, int(h), int(w)) for h, w in ab[e]]
        for b in range(32):
            low = [pts.index(x[:3]) for x in ent[off[b]:off[b + 1]]]
            assert all(x[0] * 16 + (x[1] % 4) * 4 + x[2] % 4 == b for x in ent[off[b]:off[b + 1]])
            assert low == sorted(low)
        # second order: the same entries, strictly ascending in (h, channel, w) -- the (ky, c, kx) order of a window's taps
        ent2 = [(int(w >> 16) & 15, int(w) & 255, int(w >> 8) & 255, int(w >> 20)) for w in rec[LIST2:LIST2 + n]]
        assert sorted(ent2) == sorted(ent) and not rec[LIST2 + n:].any()
        keys = [(x[1], x[0], x[2]) for x in ent2]
        assert all(a < b for a, b in zip(keys, keys[1:]))
        # pm: a conv1 pixel is touched when its 8 x 8 window (stride 4) holds a non-zero count
        both = grid.sum(axis=0)
        for p in range(400):
            oy, ox = divmod(p, 20)
            assert bool((rec[PM + p // 32] >> (p % 32)) & 1) == bool(both[4 * oy:4 * oy + 8, 4 * ox:4 * ox + 8].any()), (e, p)
        assert not (rec[PM + 12] >> 16)
        # agent tables: a candidate is a conv1 pixel whose window holds the agent's own pixel, with the tap it has there
        seen = []
        for cand in range(40):
            a, px = cand // 4, int(rec[PIX + cand])
            ph, pw = int(pos[e, a, 0]), int(pos[e, a, 1])
            if px == 0xFFFFFFFF:
                assert by[CSLOT * 4 + cand] == 255
                continue
            p, tap = px & 0xFFFF, px >> 16
            oy, ox = divmod(p, 20)
            assert (4 * oy + tap // 8, 4 * ox + tap % 8) == (ph, pw) and tap < 64
            if p not in seen:
                seen.append(p)
            assert by[CSLOT * 4 + cand] == seen.index(p) and half[SLOTPIX * 2 + seen.index(p)] == p
        assert nslots == len(seen)
        # ... and none is missing: every in-range window over the agent's pixel is a candidate
        for a in range(10):
            ph, pw = int(pos[e, a, 0]), int(pos[e, a, 1])
            want = {oy * 20 + ox for oy in range(20) for ox in range(20) if 0 <= ph - 4 * oy < 8 and 0 <= pw - 4 * ox < 8}
            got = {int(rec[PIX + a * 4 + c]) & 0xFFFF for c in range(4) if rec[PIX + a * 4 + c] != 0xFFFFFFFF}
            assert want == got


def test_record_of_the_edge_states():
    rng = np.random.RandomState(2)
    r = record_numpy(*crafted("one_bin", rng))
    assert r[0] & 0xFFFF == 1 | (11 << 8) and r[LIST] >> 20 == 80
    r = record_numpy(*crafted("all_outside", rng))
    assert r[0] & 0xFFFF == 0 and not r[1:PIX].any() and not r[PM:].any() and 1 <= r[0] >> 16 <= 4      # the rim's corners: at most four distinct pixels
    lb, ab, pos = crafted("one_tap_class", rng)
    r = record_numpy(lb, ab, pos)
    off = r.view(np.uint8)[OFF * 4:OFF * 4 + 33]
    assert len(set(off[:17])) == 2 and len(set(off[16:])) == 2          # one non-empty bucket per channel
    r = record_numpy(*crafted("two_agents_one_pixel", rng))
    cs = r.view(np.uint8)[CSLOT * 4:CSLOT * 4 + 40]
    assert (cs[8:12] == cs[28:32]).all() and (r[PIX + 8:PIX + 12] == r[PIX + 28:PIX + 32]).all()      # agents 2 and 7: same pixels, same taps
    assert (cs[12:16] == cs[16:20]).all() and (r[PIX + 12:PIX + 16] != r[PIX + 16:PIX + 20]).all()    # agents 3 and 4: same pixels, other taps
    lb, ab, pos = crafted("agent_on_locust_bin", rng)
    r = record_numpy(lb, ab, pos)
    n0, n = int(r[0] & 255), int((r[0] >> 8) & 255)
    ent = [(int(w >> 16) & 15, int(w) & 255, int(w >> 8) & 255) for w in r[LIST:LIST + n]]
    assert (0, lb[5, 0], lb[5, 1]) in ent and (1, lb[5, 0], lb[5, 1]) in ent and n - n0 == len({tuple(x) for x in ab if x[0] != 255})


# ------------------------------------------------------------------------------------------ on the device
def _train_inputs(E, seed):
    rng = np.random.RandomState(seed)
    n = E * 10
    return rng.normal(size=(n, 2)).astype(np.float32) * 0.7, (rng.normal(size=n) * 0.02).astype(np.float32), \
        (-rng.rand(n) * 400).astype(np.float32)


CASES = [(1, (s,), 40960) for s in STATES] + [(37, STATES, 200), (4099, STATES, 40990)]


@pytest.mark.gpu
@pytest.mark.parametrize("E,states,chunk", CASES, ids=["%d-%s" % (E, s[0] if len(s) == 1 else "mixed") for E, s, _ in CASES])
def test_index_record_changes_nothing_but_the_work(monkeypatch, E, states, chunk):
    """1, 37 and 4 099 envs: not multiples of the index kernel's four envs per workgroup; 37 envs in two chunks of 20 and 17; 4 099
    envs in ONE chunk, more than the helpers' resident grids (workgroups stride over the envs).  One env alone is run in every state."""
    from goldsrl import _ffi, _ffi_net
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=31)
    lb, ab, pos = mixed_obs(eng, E, states, seed=100 + E)
    act, adv, y = _train_inputs(E, seed=6)
    flat = _ffi_net.glorot_uniform_flat(seed=7)
    res = {}
    for mode in ("off", "on"):
        monkeypatch.setenv("GRL_OBS_INDEX", mode)      # read when the net is created
        net = _ffi_net.ConvNet(eng, max_chunk_samples=chunk)
        net.set_params(flat)
        out = net.predict_obs(lb, ab, pos)
        stats = net.train_obs(lb, ab, pos, act, adv, y, lr=0.0, apply_update=False)
        res[mode] = (out, stats, net.get_grads().copy())
        if mode == "on":
            dev = net.debug_obs_index(lb, ab, pos)
        net.close()
    eng.close()
    for k in ("mu", "sigma", "vs"):
        assert np.array_equal(res["on"][0][k], res["off"][0][k]), k
    assert res["on"][1] == res["off"][1]
    assert np.isfinite(res["on"][2]).all() and np.abs(res["on"][2]).max() > 0
    assert np.array_equal(res["on"][2], res["off"][2])
    ref = records_numpy(lb, ab, pos)
    bad = np.argwhere(dev != ref)
    assert len(bad) == 0, "record differs from the numpy restatement at (env, word) %s ..." % bad[:8].tolist()
