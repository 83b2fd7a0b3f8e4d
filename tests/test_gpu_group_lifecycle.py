"""The ways a sweep group ends.  A seeded random walk over the C ABI -- submissions into free slots, into slots that are members
of the open group and into slots still pending, reads, drops, flushes, synchronous runs and every setter that closes a group --
against a small host model of the state machine (prefetch_pair, sgbm_run, slot_wait, slot_before_overwrite, vo_lookahead_drop
and the setters in openvo_amd/csrc).  After every operation the model predicts the number of open members and all four closure
counters of vo_sweep_group_stats exactly; every disparity read equals the oracle's for that pair under the parameters in force
when it was submitted.  And the ORB chain of a look-ahead pair, which is enqueued when its group closes."""
import collections

import numpy as np
import pytest

from openvo_amd import _native
from tests.group_inputs import Coverage, disp16, pair, params

pytestmark = pytest.mark.gpu

N_SLOTS = 8
STEPS = 160
N_PAIRS = 24                                       # pairs per shape: a group's members and what any slot held before differ
SHAPES = [(160, 50), (176, 50), (48, 50)]          # two geometries that defer (W1 = 96, 112) and one with W1 <= 0, which never does
PARAM_SETS = [params(64), params(64, P1=100, P2=1000), params(64, speckle=0, uniquenessRatio=5)]
CAUSES = ("full", "refill of a member", "engine already a member", "other geometry", "drop", "consumer", "synchronous run",
          "synchronize", "flush", "set_sgbm", "set_roi", "set_lookahead_orb", "set_sweep_group", "set_engines")


class Model:
    """the open group as the library keeps it: who is a member (slot, engine), of which geometry, and what closed it so far"""

    def __init__(self, engines, size):
        self.engines, self.size, self.next_engine = engines, size, 0
        self.members, self.geometry = [], None
        self.closed = dict(full=0, consumer=0, flush=0, other=0)
        self.causes = collections.Counter()

    def group_size(self):
        return min(self.size, self.engines)               # an engine holds one member at a time

    def close(self, counter, cause):
        if self.members:                                  # (an empty group counts no closure)
            self.closed[counter] += 1
            self.causes[cause] += 1
            self.members = []

    def has_slot(self, slot):
        return any(s == slot for s, _ in self.members)

    def has_engine(self, engine):
        return any(e == engine for _, e in self.members)

    def prefetch(self, slot, geometry, defers):
        engine = self.next_engine
        if self.has_slot(slot):
            self.close("consumer", "refill of a member")
        elif self.has_engine(engine):
            self.close("other", "engine already a member")
        self.next_engine = (engine + 1) % self.engines
        if defers and self.group_size() > 1:
            if self.members and self.geometry != geometry:
                self.close("other", "other geometry")
            self.members.append((slot, engine))
            self.geometry = geometry
            if len(self.members) >= self.group_size():
                self.close("full", "full")

    def consume(self, slot, cause="consumer"):
        if self.has_slot(slot):
            self.close("consumer", cause)

    def synchronous_run(self):
        if self.has_engine(0):                            # engine 0 works in the main workspace
            self.close("consumer", "synchronous run")

    def set_engines(self, n):
        self.close("other", "set_engines")
        self.engines = n
        self.next_engine %= n

    def expect(self):
        return dict(self.closed, open=len(self.members))


@pytest.fixture(scope="module")
def cov(oracle):
    return Coverage(oracle)


def _walk(ctx, cov, oracle, rng, model, steps):
    filled = {}                                            # slot -> (w, h, oracle disparity of what was submitted last)
    serial = [0]
    current = {"p": PARAM_SETS[0]}
    ctx.set_sgbm(current["p"])
    assert ctx.set_sweep_group(model.size) == model.group_size()

    def fresh(w, h):
        """the next pair of a shape and its oracle disparity under the parameters in force"""
        serial[0] += 1
        p = current["p"]
        k = serial[0] % N_PAIRS
        if w - p["numDisparities"] <= 0:                   # nothing to compute: no coverage conditions either
            L, R = pair(w, h, k, p["numDisparities"], 0)
            return L, R, oracle.sgbm_compute(L, R, p, 0)
        c = cov.get(w, h, k, p)
        assert c["lr_px"] >= 1, ("pixels the left-right check removes", w, h, k, p)      # (per member: so in every group)
        return c["L"], c["R"], c["ref"]

    def read(slot):
        w, h, ref = filled[slot]
        got = disp16(ctx, slot, w, h)
        assert np.array_equal(got, ref), ("slot", slot, (w, h), "pixels off", int((got != ref).sum()))

    def any_slot():
        """a filled slot; every other time one of the open group's, if there is one"""
        pool = [s for s, _ in model.members] if model.members and rng.random() < 0.5 else sorted(filled)
        return pool[int(rng.integers(len(pool)))]

    ops = ["prefetch"] * 14 + ["read"] * 3 + ["drop", "drop", "flush", "synchronize", "sync_run", "sync_run", "set_sgbm", "set_roi", "set_lookahead_orb",
                                              "set_sweep_group", "set_engines"]
    orb_on = False
    for step in range(steps):
        op = ops[int(rng.integers(len(ops)))]
        if op in ("read", "drop") and not filled:
            op = "prefetch"
        if op == "prefetch":
            slot = int(rng.integers(N_SLOTS))
            # (with a group open: mostly its geometry or the one that never defers -- pairs that pass the open group by and
            #  move the round-robin engine on to one that holds a member)
            w, h = SHAPES[int(rng.choice([0, 0, 0, 1, 2, 2]))] if not model.members or rng.random() < 0.3 else \
                (model.geometry if rng.random() < 0.5 else SHAPES[2])
            L, R, ref = fresh(w, h)
            ctx.prefetch_pair(slot, L, R, True)
            filled[slot] = (w, h, ref)
            model.prefetch(slot, (w, h), defers=w - current["p"]["numDisparities"] > 0)
            for s, _ in model.members:                     # no two members of the open group with one disparity
                assert s == slot or not np.array_equal(filled[s][2], ref), (step, "two members alike", s, slot)
        elif op == "read":
            slot = any_slot()
            model.consume(slot)
            read(slot)
        elif op == "drop":
            slot = any_slot()
            ctx.lookahead_drop(slot)
            model.consume(slot, "drop")
        elif op == "flush":
            ctx.lookahead_flush()
            model.close("flush", "flush")
        elif op == "synchronize":
            ctx.synchronize()
            model.close("consumer", "synchronize")
        elif op == "sync_run":
            L, R, ref = fresh(*SHAPES[int(rng.integers(2))])
            got = ctx.sgbm_compute_host(L, R)
            model.synchronous_run()
            assert np.array_equal(got, ref), ("synchronous run", step, int((got != ref).sum()))
        elif op == "set_sgbm":
            current["p"] = PARAM_SETS[int(rng.integers(len(PARAM_SETS)))]
            ctx.set_sgbm(current["p"])
            model.close("other", "set_sgbm")
        elif op == "set_roi":
            ctx.set_roi(int(rng.integers(0, 8)), int(rng.integers(0, 4)), int(rng.integers(100, 200)), int(rng.integers(40, 60)))
            model.close("other", "set_roi")
        elif op == "set_lookahead_orb":
            orb_on = not orb_on
            if orb_on:
                ctx.lookahead_orb(50, 1, 16, 16 * 1000)
            else:
                ctx.lookahead_orb_off()
            model.close("other", "set_lookahead_orb")
        elif op == "set_sweep_group":
            model.close("other", "set_sweep_group")
            model.size = int(rng.choice([2, 3, 4]))
            assert ctx.set_sweep_group(model.size) == model.group_size()
        elif op == "set_engines":
            model.set_engines(int(rng.choice([3, 5])))
            assert ctx.set_engines(model.engines) == model.engines
        assert ctx.sweep_group_stats() == model.expect(), (step, op, ctx.sweep_group_stats(), model.expect())
    ctx.lookahead_flush()
    model.close("flush", "flush")
    assert ctx.sweep_group_stats() == model.expect()
    for slot in sorted(filled):
        read(slot)


@pytest.mark.parametrize("seed,engines,size", [(5, 3, 3), (25, 5, 4)])
def test_random_walk_over_the_abi_against_the_host_model(oracle, cov, seed, engines, size):
    """engines and group size are where the walk starts: set_engines (3 / 5) and set_sweep_group (2 / 3 / 4) are among its steps"""
    rng = np.random.default_rng(seed)
    model = Model(engines, size)
    ctx = _native.Context(0, 176, 64, 64, 64, engines=engines)
    try:
        _walk(ctx, cov, oracle, rng, model, STEPS)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()
    missing = [c for c in CAUSES if not model.causes[c]]
    assert not missing, (missing, dict(model.causes))


def _keypoints(ctx, slot, args):
    k = ctx.orb_slot(slot, *args)
    return {name: v.copy() for name, v in k.items()}


def test_orb_chain_of_a_look_ahead_pair_in_a_group(oracle, cov):
    """vo_set_lookahead_orb with the fused disparity mask and a group of 3: every member's ORB chain runs on its own engine's
    stream behind the group's post filters.  The group comes first, on a fresh context: no slot, engine or workspace holds an
    earlier answer that a chain started too early, or never, could pass off as its own.  Keypoints and descriptors of every
    member equal the oracle's on the mask of the oracle's disparity, and those of the same pairs at group size 1 -- submitted
    afterwards, into other slots and each on another engine -- bit for bit."""
    w, h, D = 224, 96, 64
    p = params(D)
    orb = (300, 1, 16, 16 * 40)
    members = cov.group(w, h, [0, 1, 2], p)
    ctx = _native.Context(0, w, h, D, 300, engines=3)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*orb)
        got = {}
        for B, slot0, order in ((3, 2, (0, 1, 2)), (1, 10, (1, 2, 0))):
            assert ctx.set_sweep_group(B) == B
            for n, i in enumerate(order):
                ctx.prefetch_pair(slot0 + i, members[i]["L"], members[i]["R"], True)
                assert ctx.sweep_group_stats()["open"] == (n + 1 if B > 1 and n + 1 < B else 0)
            got[B] = [(_keypoints(ctx, slot0 + i, orb), disp16(ctx, slot0 + i, w, h)) for i in reversed(range(3))][::-1]
        st = ctx.sweep_group_stats()
        assert (st["full"], st["consumer"], st["flush"], st["other"], st["open"]) == (1, 0, 0, 0, 0)
        for i, m in enumerate(members):
            (k1, d1), (k3, d3) = got[1][i], got[3][i]
            assert np.array_equal(d3, m["ref"]) and np.array_equal(d1, m["ref"]), i
            assert len(k3["xy"]) > 50, (i, len(k3["xy"]))
            mask = ((m["ref"] >= orb[2]) & (m["ref"] <= orb[3])).astype(np.uint8) * 255
            assert 0 < (mask == 0).sum() < mask.size
            ref = oracle.orb_detect_and_compute(m["L"], mask, orb[0])
            for name in ("xy", "angle", "octave", "desc"):
                assert ref[name].shape == k3[name].shape and np.array_equal(ref[name].view(np.uint8), k3[name].view(np.uint8)), (i, name)
            for name in k1:
                assert k1[name].shape == k3[name].shape and np.array_equal(k1[name].view(np.uint8), k3[name].view(np.uint8)), (i, name)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()
