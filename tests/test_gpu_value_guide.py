"""Cost-to-go guidance inside the step (``pw_guide_step`` / ``guide.ValueGuide`` / ``VecPushWorld.set_guide``)
against the numpy restatement (tests/value_guide_restatement.py) whose lookup is the host reference of
tests/test_gpu_solution_batch.py.  Integers are compared exactly and the shaped reward bit for bit."""
import numpy as np
import pytest
import torch

import value_guide_restatement as VR
from test_gpu_solution_batch import BEYOND, CASES, NINE, SEVEN, World
from test_gpu_solution_table import INF

pytestmark = pytest.mark.gpu

GAMMA, SCALE = 0.99, 0.1  # neither is representable: a multiply-add contracted into one rounding shows in the last bit
NO_TABLE = CASES.index("rand:42")  # left out of every build: a puzzle of the set without a table
FLAGS = VR.AUTORESET | VR.END_DEAD


def _np(t):
    return t.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _lookup(w):
    """The restatement's lookup over the world's host tables, ``NO_TABLE`` left out as in the library's builds."""
    return VR.HostLookup({p: (w.hosts[p], *w.dims[p]) for p in range(len(w.keys)) if p != NO_TABLE})


def _dead_cost(w):
    dc = np.zeros(len(w.all_keys), dtype=np.int32)
    for p, h in enumerate(w.hosts):
        if p != NO_TABLE:
            dc[p] = h.summary[3] + 1
    return dc


# ---- 1. the rule, branch by branch ---------------------------------------------------------------------------------------------
def _items(w, npad):
    """Rule inputs built from the host tables, per puzzle: every branch of the rule by construction.  Returns a list of
    dicts (p, state, prev, seen, term, trunc, reward, mask, kind)."""
    rng = np.random.default_rng(2028)
    items = []

    def add(p, state, prev, kind, seen=0, term=0, trunc=0, reward=-0.01, mask=1):
        items.append(dict(p=p, state=state, prev=prev, seen=seen, term=term, trunc=trunc, reward=reward, mask=mask, kind=kind))

    def cost_of(h, i):
        return -1 if h.cost[i] == INF else int(h.cost[i])

    for p, h in enumerate(w.hosts):
        W, H = w.dims[p]
        N = len(h.states[0])
        fin = np.flatnonzero(h.cost != INF)
        dead_succ = [(i, a) for i in fin[:4000] for a in range(4) if h.cost[h.succ[i, a]] == INF]
        for i, a in dead_succ[:12]:  # a finite cost stepped into a dead end: cut
            add(p, h.states[h.succ[i, a]], int(h.cost[i]), "dead_entered")
        for i in np.flatnonzero(h.cost == 1)[:4]:  # cost 1 stepped into the goal
            a = int(np.flatnonzero([h.acts[i] >> k & 1 for k in range(4)])[0])
            add(p, h.states[h.succ[i, a]], 1, "goal", term=1, reward=10.0)
        for i in (rng.choice(fin, size=100) if len(fin) else ()):  # any action from a solvable state
            a = int(rng.integers(0, 4))
            add(p, h.states[h.succ[i, a]], int(h.cost[i]), "step")
        for i in rng.choice(len(h.states), size=12):
            i = int(i)
            add(p, h.states[i], int(rng.integers(0, 9)), "fresh", seen=1)                       # the step reset it
            add(p, h.states[i], cost_of(h, i), "refused", term=0xFF, trunc=0xFF, reward=0.0)    # an action >= 4
            add(p, h.states[i], cost_of(h, i), "masked", mask=0)
            add(p, h.states[i], -2, "prev_unknown")
            add(p, h.states[i], cost_of(h, i), "truncated", trunc=1)                            # max_steps: never cut
        for i in np.flatnonzero(h.cost == INF)[:3]:  # stays inside a dead end with no flag: cut, not "entered"
            add(p, h.states[int(i)], -1, "dead_stays")
        s = [list(xy) for xy in h.states[int(rng.integers(0, len(h.states)))]]
        s[p % N][p % 2] = (H if p % 2 else W) if p % 3 == 0 else [-1, 16, -128, 127, 100, -2, 64, 31, 17, 20][p]
        add(p, tuple(tuple(xy) for xy in s), 3, "off_grid")
        for _ in range(1000):  # a state inside the grid that the start does not reach
            s = tuple((int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(N))
            if s not in h.index:
                add(p, s, 2, "unreachable")
                break
    for p in range(len(w.keys), len(w.all_keys)):  # beyond the kernel's limits: no table
        add(p, ((1, 1),), 4, "foreign")
    add(-1, ((1, 1),), 4, "outside_set")
    add(len(w.all_keys), ((1, 1),), -1, "outside_set")
    return items


def _arrays(items, npad, seed=5):
    rng = np.random.default_rng(seed)
    n = len(items)
    pos = rng.integers(-128, 128, size=(n, npad, 2)).astype(np.int8)  # garbage beyond each puzzle's movables
    for i, it in enumerate(items):
        pos[i, :len(it["state"])] = np.array(it["state"], dtype=np.int64).astype(np.int8)
    col = lambda k, dt: np.array([it[k] for it in items], dtype=dt)  # noqa: E731
    return dict(puzzle_id=col("p", np.int32), pos=pos, cost=col("prev", np.int32), seen=col("seen", np.uint8),
                terminated=col("term", np.uint8), truncated=col("trunc", np.uint8), reward=col("reward", np.float64),
                mask=col("mask", np.uint8))


def _run_raw(w, tabs, a, flags, dead_cost, cost_in=None, acts_in=None, shaping=True, counting=True):
    """One ``pw_guide_step`` over the arrays ``a`` through the engine wrapper; returns the outputs as numpy."""
    dev, n = w.eng.device, len(a["puzzle_id"])
    d = {k: torch.as_tensor(v).to(dev) for k, v in a.items()}
    acts = torch.full((n,), 0xAB, dtype=torch.uint8, device=dev)
    dead = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    shaped = torch.full((n,), 123.0, dtype=torch.float64, device=dev) if shaping else None
    counts = torch.zeros((len(w.all_keys), 4), dtype=torch.int64, device=dev) if counting else None
    before = w.eng.counters()["episodes_ended"]
    w.eng.guide_step(tabs.handle if cost_in is None else None, cost_in, acts_in, d["puzzle_id"], d["pos"], d["reward"],
                     d["terminated"], d["truncated"], d["mask"], d["cost"], acts, d["seen"], dead, shaped,
                     torch.as_tensor(dead_cost).to(dev), GAMMA, SCALE, counts, flags)
    out = dict(cost=_np(d["cost"]), acts=_np(acts), dead=_np(dead), seen=_np(d["seen"]), truncated=_np(d["truncated"]),
               shaped=None if shaped is None else _np(shaped), counts=None if counts is None else _np(counts),
               ended=w.eng.counters()["episodes_ended"] - before)
    assert (_np(d["reward"]) == a["reward"]).all() and (_np(d["terminated"]) == a["terminated"]).all()  # read only
    return out


def _want(look, a, flags, dead_cost):
    n = len(a["puzzle_id"])
    return VR.guide_step(look, a["puzzle_id"], a["pos"], a["reward"], a["terminated"], a["truncated"], a["cost"],
                         np.full(n, 0xAB, np.uint8), a["seen"], np.full(n, 7, np.uint8), dead_cost, GAMMA, SCALE, flags,
                         mask=a["mask"], shaped=np.full(n, 123.0))


def _compare(got, want, tag):
    for k in ("cost", "acts", "dead", "seen", "truncated", "counts"):
        assert (got[k] == want[k]).all(), (tag, k, np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(1))[:8])
    assert (_bits(got["shaped"]) == _bits(want["shaped"])).all(), (tag, "shaped")
    assert got["ended"] == want["ended"], tag


@pytest.mark.parametrize("npad, extra", [(4, [BEYOND]), (8, [SEVEN]), (16, [SEVEN, NINE])])
def test_the_rule_branch_by_branch(golden, npad, extra):
    from pushworld_amd.search import SolutionTableBatch

    w = World(golden, extra)
    assert w.eng.np == npad
    tabs = SolutionTableBatch(w.eng, [i for i in range(len(w.all_keys)) if i != NO_TABLE])
    try:
        look, dc = _lookup(w), _dead_cost(w)
        items = _items(w, npad)
        assert 1200 < len(items) < 2600, len(items)  # the mixed batch of about 2 000
        by_puzzle = sorted(items, key=lambda it: it["p"])  # 64 and more consecutive environments of one puzzle
        order = np.random.default_rng(1).permutation(len(items))
        cycled = [items[i] for i in order]                 # the ids change from lane to lane
        for name, layout in (("by puzzle", by_puzzle), ("cycled", cycled)):
            a = _arrays(layout, npad)
            want = _want(look, a, FLAGS, dc)
            # a condition on the INPUTS, checked on the host: every branch of the rule occurs
            br = want["branches"]
            assert all(br[k] > 0 for k in ("masked", "fresh", "refused", "cut", "guided", "optimal", "dead_entered", "unknown",
                                           "shaped_nonzero")), br
            kinds = {it["kind"] for it in layout}
            assert {"dead_entered", "goal", "fresh", "refused", "unreachable", "off_grid", "foreign", "masked", "dead_stays",
                    "outside_set", "prev_unknown", "truncated"} <= kinds
            assert (want["cost"][[it["kind"] == "goal" for it in layout]] == 0).all()
            assert (want["cost"][[it["kind"] in ("unreachable", "off_grid", "foreign", "outside_set") for it in layout]] == -2).all()
            assert want["cost"][[it["p"] == NO_TABLE and it["mask"] == 1 for it in layout]].tolist().count(-2) > 10
            assert br["cut"] > br["dead_entered"] > 0 and want["counts"][NO_TABLE, VR.GUIDED] == 0
            if name == "by puzzle":  # the counted lanes of some wavefront share a puzzle, and of some other they do not
                ids = a["puzzle_id"]
                waves = [ids[k:k + 64] for k in range(0, len(ids), 64)]
                assert any(len(set(x.tolist())) == 1 for x in waves) and any(len(set(x.tolist())) > 1 for x in waves)
            _compare(_run_raw(w, tabs, a, FLAGS, dc), want, (name, "all"))
            for flags in (0, VR.AUTORESET, VR.END_DEAD, VR.REFRESH, VR.REFRESH | FLAGS):
                want_f = _want(look, a, flags, dc)
                got_f = _run_raw(w, tabs, a, flags, dc)
                if flags & VR.REFRESH:
                    assert want_f["ended"] == 0 and want_f["counts"].sum() == 0 and (want_f["shaped"] == 123.0).all()
                _compare(got_f, want_f, (name, flags))
            # without shaped and counts the rest is the same
            bare = _run_raw(w, tabs, a, FLAGS, dc, shaping=False, counting=False)
            for k in ("cost", "acts", "dead", "seen", "truncated", "ended"):
                assert np.all(bare[k] == want[k]), (name, "bare", k)
        # batch sizes around the wavefront: one puzzle throughout, and ids cycling per lane
        one = [it for it in items if it["p"] == 1]
        for n in (1, 63, 64, 65, 257):
            for name, layout in (("one puzzle", (one * (n // len(one) + 1))[:n]), ("cycled", cycled[:n])):
                a = _arrays(layout, npad, seed=n)
                _compare(_run_raw(w, tabs, a, FLAGS, dc), _want(look, a, FLAGS, dc), (name, n))
    finally:
        tabs.close()


# ---- 2. fused form against applied form, through ValueGuide --------------------------------------------------------------------
def _feed(vec, guide, a):
    """Puts the rule inputs ``a`` into the environment and the guide as a step would have left them."""
    dev = vec.device
    vec.pos.copy_(torch.as_tensor(a["pos"]).to(dev))
    vec.reward.copy_(torch.as_tensor(a["reward"]).to(dev))
    vec.terminated.copy_(torch.as_tensor(a["terminated"]).to(dev))
    vec.truncated.copy_(torch.as_tensor(a["truncated"]).to(dev))
    guide.cost.copy_(torch.as_tensor(a["cost"]).to(dev))
    guide.seen.copy_(torch.as_tensor(a["seen"]).to(dev))
    guide.counts.zero_()


def _guide_out(vec, guide):
    return dict(cost=_np(guide.cost), acts=_np(guide.acts), dead=_np(guide.dead), seen=_np(guide.seen),
                truncated=_np(vec.truncated), shaped=_np(guide.shaped), counts=_np(guide.counts))


def test_fused_form_equals_applied_form(golden):
    from pushworld_amd.guide import ValueGuide
    from pushworld_amd.vec_env import VecPushWorld

    w = World(golden, [SEVEN])
    items = [it for it in _items(w, 8) if 0 <= it["p"] < len(w.all_keys)]
    a = _arrays(items, 8)
    a["mask"][:] = 1  # (the step path has no mask)
    n = len(items)
    vec = VecPushWorld(w.pset, n, puzzle_ids=a["puzzle_id"], observation=None, max_steps=50, autoreset=True, bind=False)
    tabs = vec.solution_tables([i for i in range(len(w.all_keys)) if i != NO_TABLE])
    single = vec.solution_table(NO_TABLE)
    try:
        kw = dict(gamma=GAMMA, scale=SCALE, end_dead=True)
        fused, applied = ValueGuide(vec, tabs, **kw), ValueGuide(vec, [tabs, single], **kw)
        assert fused.fused and not applied.fused and fused.level == applied.level == "move"
        dc = _dead_cost(w)
        assert (_np(fused.dead_cost) == dc).all()  # the default: largest finite cost + 1, 0 without a table
        dc_applied = dc.copy()
        dc_applied[NO_TABLE] = w.hosts[NO_TABLE].summary[3] + 1
        assert (_np(applied.dead_cost) == dc_applied).all()
        vec.reset()
        outs = []
        for guide in (fused, applied):
            _feed(vec, guide, a)
            guide.step()
            outs.append(_guide_out(vec, guide))
        assert (_np(applied._cost_in) == -2).all() and (_np(applied._acts_in) == 0).all()  # cleared behind the read
        want = _want(_lookup(w), a, FLAGS, dc)
        for k in ("cost", "acts", "dead", "seen", "truncated", "counts"):
            assert (outs[0][k] == want[k]).all(), k
        assert (_bits(outs[0]["shaped"]) == _bits(want["shaped"])).all()
        covered = a["puzzle_id"] != NO_TABLE  # where both cover, the two forms agree in every output
        for k in ("cost", "acts", "dead", "seen", "truncated"):
            assert (outs[0][k][covered] == outs[1][k][covered]).all(), k
        assert (_bits(outs[0]["shaped"])[covered] == _bits(outs[1]["shaped"])[covered]).all()
        rows = np.arange(len(w.all_keys)) != NO_TABLE
        assert (outs[0]["counts"][rows] == outs[1]["counts"][rows]).all()
        # ... and the applied form knows the left-out puzzle: the whole world is the restatement's with its table added
        full = VR.HostLookup({p: (w.hosts[p], *w.dims[p]) for p in range(len(w.keys))})
        want = _want(full, a, FLAGS, dc_applied)
        for k in ("cost", "acts", "dead", "seen", "truncated", "counts"):
            assert (outs[1][k] == want[k]).all(), k
        assert (_bits(outs[1]["shaped"]) == _bits(want["shaped"])).all()
        assert (outs[1]["cost"][~covered] != -2).any() and (outs[0]["cost"][~covered] == -2).all()
        # a masked refresh touches the masked environments only
        _feed(vec, applied, a)
        mask = torch.as_tensor((np.arange(n) % 3 == 0)).to(vec.device)
        applied.refresh(mask)
        got = _guide_out(vec, applied)
        want = _want(full, dict(a, mask=_np(mask).astype(np.uint8)), VR.REFRESH, dc_applied)
        assert (got["cost"] == want["cost"]).all() and (got["seen"] == want["seen"]).all() and got["counts"].sum() == 0
        assert (_np(applied._cost_in) == -2).all()
    finally:
        single.close()
        tabs.close()


# ---- 3. sixty random steps ------------------------------------------------------------------------------------------------------
def _precut(trunc, steps, max_steps):
    """``truncated`` as the step launch left it: a flag of 1 below ``max_steps`` can only be the guide's cut."""
    return np.where((trunc == 1) & (steps < max_steps), 0, trunc).astype(np.uint8)


def test_sixty_random_steps(golden):
    from pushworld_amd.vec_env import VecPushWorld

    w = World(golden, [BEYOND])
    B, T, max_steps, P = 300, 60, 30, len(w.all_keys)
    ids = (np.arange(B) % P).astype(np.int32)
    vec = VecPushWorld(w.pset, B, puzzle_ids=ids, observation=None, max_steps=max_steps, autoreset=True, episode_stats=True)
    tabs = vec.solution_tables([i for i in range(P) if i != NO_TABLE])
    try:
        guide = vec.set_guide(tabs, gamma=GAMMA, scale=SCALE, end_dead=True)
        assert vec.guide is guide and vec.cost is guide.cost and vec.dead is guide.dead and vec.shaped_reward is guide.shaped
        with pytest.raises(RuntimeError, match="rollout"):
            vec.rollout(torch.zeros((2, B), dtype=torch.uint8, device=vec.device))
        look, dc = _lookup(w), _dead_cost(w)
        vec.reset()
        vec.counters_reset()
        start = np.array([w.hosts[p].summary[4] if p < len(w.keys) and p != NO_TABLE else -2 for p in ids])
        assert (_np(vec.cost) == start).all() and (_np(guide.seen) == 0).all()  # reset refreshed the guide
        rng = np.random.default_rng(9)
        counts = np.zeros((P, 4), dtype=np.int64)
        episodes, ended, cuts, cut_prev = np.zeros(P, dtype=np.int64), 0, 0, np.zeros(B, dtype=bool)
        for t in range(T):
            prev_cost, prev_seen = _np(guide.cost), _np(guide.seen)
            actions = rng.integers(0, 4, size=B).astype(np.uint8)
            actions[rng.integers(0, B, size=2)] = 4 + t % 3  # refused: flags 0xFF
            vec.step(torch.as_tensor(actions).to(vec.device))
            steps, term, trunc = _np(vec.steps), _np(vec.terminated), _np(vec.truncated)
            assert (steps[cut_prev] == 0).all() and (trunc[cut_prev] == 0).all(), t  # every cut environment was reset
            want = VR.guide_step(look, ids, _np(vec.pos), _np(vec.reward), term, _precut(trunc, steps, max_steps), prev_cost,
                                 np.zeros(B, np.uint8), prev_seen, np.zeros(B, np.uint8), dc, GAMMA, SCALE, FLAGS, counts=counts)
            got = _guide_out(vec, guide)
            for k in ("cost", "acts", "dead", "seen", "truncated", "counts"):
                assert (got[k] == want[k]).all(), (t, k)
            assert (_bits(got["shaped"]) == _bits(want["shaped"])).all(), t
            counts = want["counts"]
            cut_prev = (trunc == 1) & (steps < max_steps)
            cuts += int(cut_prev.sum())
            assert cut_prev.sum() == want["ended"]
            flagged = ((term | trunc) != 0) & (term != 0xFF)
            np.add.at(episodes, ids[flagged], 1)
            ended += int(flagged.sum())
        assert cuts > 20 and counts[:, VR.DEAD_ENTERED].sum() > 20 and counts[:, VR.OPTIMAL].sum() > 0
        st = vec.puzzle_stats()
        assert (st.episodes == episodes).all() and st.episodes.sum() == ended  # a cut episode is counted in the same call
        assert vec.counters()["episodes_ended"] == ended
        gs = guide.stats()
        assert (gs.guided == counts[:, 0]).all() and (gs.dead_entered == counts[:, 2]).all()
        # set_states and set_puzzle_ids refresh; set_guide(None) removes
        pos = _np(vec.pos).copy()
        pos[:, 0] = (1, 1)
        vec.set_states(pos)
        want = VR.guide_step(look, ids, pos, _np(vec.reward), _np(vec.terminated), _np(vec.truncated), _np(guide.cost),
                             _np(guide.acts), _np(guide.seen), _np(guide.dead), dc, GAMMA, SCALE, VR.REFRESH)
        assert (_np(vec.cost) == want["cost"]).all() and (_np(guide.counts) == counts).all()
        assert vec.set_guide(None) is None and vec.guide is None and vec._call_guide is None and vec.cost is None
    finally:
        tabs.close()


# ---- 4. with a start pool: the launch order --------------------------------------------------------------------------------------
def test_a_drawn_start_state_carries_its_cost(golden):
    from pushworld_amd.start_pool import StartPool
    from pushworld_amd.vec_env import VecPushWorld

    w = World(golden, [BEYOND])
    B, P = 256, len(w.all_keys)
    ids = (np.arange(B) % P).astype(np.int32)
    kw = dict(puzzle_ids=ids, observation=None, max_steps=4, autoreset=True)
    maker = VecPushWorld(w.pset, 4, observation=None)
    made = maker.solution_tables([i for i in range(P) if i != NO_TABLE])
    pool = StartPool.from_tables(maker, [made], max_per_level=8)
    made.close()
    vec = VecPushWorld(w.pset, B, start_pool=pool, start_band=(1, None), **kw)
    tabs = vec.solution_tables([i for i in range(P) if i != NO_TABLE])
    try:
        vec.set_guide(tabs, end_dead=True)
        vec.reset()
        initial = np.array([w.hosts[p].summary[4] if p < len(w.keys) and p != NO_TABLE else -2 for p in ids])
        level = _np(vec.start_level)
        assert (_np(vec.cost) == np.where(level >= 0, level, initial)).all() and (level >= 1).sum() > B // 2
        rng, fresh_seen = np.random.default_rng(3), 0
        for t in range(12):
            was_done = (_np(vec.terminated) | _np(vec.truncated)) != 0
            vec.step(torch.as_tensor(rng.integers(0, 4, size=B).astype(np.uint8)).to(vec.device))
            level, cost = _np(vec.start_level), _np(vec.cost)
            # the guide ran behind the draw: a fresh environment already carries the cost of the state it drew
            assert (cost[was_done] == np.where(level >= 0, level, initial)[was_done]).all(), t
            assert (_np(vec.steps)[was_done] == 0).all() and (_np(vec.truncated)[was_done] == 0).all()  # fresh: never cut
            fresh_seen += int((was_done & (level >= 1)).sum())
        assert fresh_seen > B
    finally:
        tabs.close()


# ---- 5. push-level tables, applied form, behind step_push_mask --------------------------------------------------------------------
def test_push_tables_behind_step_push_mask(golden):
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.vec_env import VecPushWorld

    keys = ["pytest:trivial_tool.pwp", "l0:level0/base/train/level_0_base_train_0.pwp", "pytest:transitive_pushing.pwp", "rand:3"]
    puzzles = [PushWorldPuzzle(text=golden.text(k)) for k in keys]
    B, max_steps = 128, 40
    ids = (np.arange(B) % 4).astype(np.int32)
    vec = VecPushWorld(puzzles, B, puzzle_ids=ids, observation=None, max_steps=max_steps, autoreset=True)
    tabs = vec.push_tables()
    try:
        guide = vec.set_guide([tabs], gamma=GAMMA, scale=SCALE, end_dead=True)
        assert guide.level == "push" and not guide.fused
        dc = _np(guide.dead_cost)
        status, mc = _np(tabs.status), _np(tabs.max_cost)
        assert dc.tolist() == [int(mc[i]) + 1 if status[i] == 0 else 0 for i in range(4)] and (status == 0).sum() >= 3
        vec.reset()
        vec.observe_pushes()
        assert (_np(vec.cost) == _np(vec.push_cost_to_go([tabs]).cost)).all()
        gen = torch.Generator(device=vec.device).manual_seed(4)
        counts, cuts = np.zeros((4, 4), dtype=np.int64), 0
        for t in range(14):
            if t == 7:  # a refresh that makes every push view stale: the environments are moved behind the step's back
                vec.set_states(_np(vec.pos)[np.roll(np.arange(B), 4)])
                assert (_np(vec.cost) == _np(vec.push_cost_to_go([tabs]).cost)).all() and (_np(guide.counts) == counts).all()
                vec.observe_pushes()
            prev_cost, prev_seen = _np(guide.cost), _np(guide.seen)
            mask = ((vec.push_view_mask.unsqueeze(1) & torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=vec.device)
                     .view(1, 4, 1, 1)) != 0).reshape(B, -1).to(torch.float32)
            has = mask.sum(1, keepdim=True) > 0
            choice = torch.multinomial(torch.where(has, mask, torch.ones_like(mask)), 1, generator=gen).squeeze(1)
            vec.step_push_mask(choice=choice)
            steps, term, trunc = _np(vec.steps), _np(vec.terminated), _np(vec.truncated)
            look = VR.ArrayLookup(_np(vec.push_cost_to_go([tabs]).cost))  # the existing query of the states the step left
            want = VR.guide_step(look, ids, _np(vec.pos), _np(vec.reward), term, _precut(trunc, steps, max_steps), prev_cost,
                                 np.zeros(B, np.uint8), prev_seen, np.zeros(B, np.uint8), dc, GAMMA, SCALE, FLAGS, counts=counts)
            got = _guide_out(vec, guide)
            for k in ("cost", "acts", "dead", "seen", "truncated", "counts"):
                assert (got[k] == want[k]).all(), (t, k)
            assert (_bits(got["shaped"]) == _bits(want["shaped"])).all(), t
            assert (got["acts"] == 0).all() and (_np(guide._cost_in) == -2).all()
            counts, cuts = want["counts"], cuts + want["ended"]
        assert counts[:, VR.GUIDED].sum() > B and counts[:, VR.OPTIMAL].sum() > 0
    finally:
        tabs.close()


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------
def test_captured_step_and_guide(golden):
    from pushworld_amd.vec_env import VecPushWorld

    w = World(golden, [BEYOND])
    B, R, P = 320, 3, len(w.all_keys)
    ids = (np.arange(B) // 32 % P).astype(np.int32)
    kw = dict(puzzle_ids=ids, observation=None, max_steps=6, autoreset=True, bind=False)
    eager, graphed = VecPushWorld(w.pset, B, **kw), VecPushWorld(w.pset, B, **kw)
    dev = eager.device
    tabs = [v.solution_tables([i for i in range(P) if i != NO_TABLE]) for v in (eager, graphed)]
    try:
        for v, tb in zip((eager, graphed), tabs):
            v.set_guide(tb, gamma=GAMMA, scale=SCALE, end_dead=True)
            v.reset()
        gen = torch.Generator(device=dev).manual_seed(8)
        acts = torch.randint(0, 4, (R + 6, B), dtype=torch.uint8, device=dev, generator=gen)
        static_actions = torch.zeros((B,), dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream(device=dev)  # warm-up on a side stream, then capture ONE step: the step and the guide launch
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for k in range(6):
                static_actions.copy_(acts[k])
                graphed.step(static_actions)
        torch.cuda.current_stream(dev).wait_stream(s)
        for k in range(6):
            eager.step(acts[k])
        g = torch.cuda.CUDAGraph()
        static_actions.copy_(acts[6])
        with torch.cuda.graph(g):
            graphed.step(static_actions)
        for r in range(R):  # (the capture itself ran nothing: the first replay is step 6)
            static_actions.copy_(acts[6 + r])
            g.replay()
            eager.step(acts[6 + r])
            for name in ("pos", "steps", "terminated", "truncated", "reward"):
                assert torch.equal(getattr(eager, name), getattr(graphed, name)), (name, r)
            for name in ("cost", "acts", "dead", "seen", "counts"):
                assert torch.equal(getattr(eager.guide, name), getattr(graphed.guide, name)), (name, r)
            assert torch.equal(eager.guide.shaped.view(torch.int64), graphed.guide.shaped.view(torch.int64)), r
        assert eager.counters() == graphed.counters() and int(eager.guide.counts[:, 0].sum()) > B
    finally:
        for tb in tabs:
            tb.close()


# ---- 7. the facades --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["gym", "dm", "push", "push_dm"])
def test_facades(golden, flavour):
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.vector_env import (PushWorldDmVectorEnv, PushWorldPushDmVectorEnv, PushWorldPushVectorEnv,
                                          PushWorldVectorEnv)

    keys = ["pytest:trivial_tool.pwp", "l0:level0/base/train/level_0_base_train_0.pwp", "pytest:transitive_pushing.pwp", "rand:3"]
    puzzles = [PushWorldPuzzle(text=golden.text(k)) for k in keys]
    cls = dict(gym=PushWorldVectorEnv, dm=PushWorldDmVectorEnv, push=PushWorldPushVectorEnv, push_dm=PushWorldPushDmVectorEnv)[flavour]
    B = 16
    env = cls(puzzles, B, max_steps=12, observation="uint8", seed=1)
    names = ("cost_to_go", "guide_actions", "dead_end", "shaped_reward")

    def extras(out):
        """(the dict that carries the guide's entries, the reward) of a reset / step result"""
        if flavour in ("gym", "push"):
            return out[-1], (out[1] if len(out) == 5 else None)
        return out.observation, out.reward

    def act():
        if flavour in ("gym", "dm"):
            return torch.full((B,), 1, dtype=torch.uint8, device=env.vec.device)
        m = env._action_mask().to(torch.float32)
        return torch.multinomial(torch.where(m.sum(1, keepdim=True) > 0, m, torch.ones_like(m)), 1).squeeze(1)

    plain, _ = extras(env.reset(seed=1))
    if flavour == "dm":
        assert isinstance(plain, torch.Tensor)  # without a guide the observation is the batch, as ever
    else:
        assert not set(names) & set(plain)
    tabs = env.vec.solution_tables()
    try:
        for shaped_on in (False, True):
            guide = env.set_guide(tabs, use_shaped_reward=shaped_on, gamma=GAMMA, scale=SCALE)
            assert guide is env.vec.guide and env.use_shaped_reward is shaped_on
            info, _ = extras(env.reset(seed=1))
            assert set(names) <= set(info) and (info["cost_to_go"] >= 0).all()
            if flavour in ("dm", "push_dm"):
                assert "board" in info
            differs = False
            for _ in range(6):
                info, reward = extras(env.step(act()))
                assert info["cost_to_go"] is guide.cost and info["guide_actions"] is guide.acts
                assert info["dead_end"] is guide.dead and info["shaped_reward"] is guide.shaped
                assert reward is (guide.shaped if shaped_on else env.vec.reward)
                differs |= not torch.equal(guide.shaped, env.vec.reward)
            assert differs
        assert env.set_guide(None) is None and env.use_shaped_reward is False
        info, reward = extras(env.step(act()))
        assert reward is env.vec.reward
        if flavour != "dm":
            assert not set(names) & set(info)
    finally:
        tabs.close()
