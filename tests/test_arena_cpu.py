"""The compact activation arena (grnet_create_ex / GRNET_CREATE_COMPACT_ARENA), checked without a GPU: the assignment on known and random
conflict graphs, an INDEPENDENT proof that the real layouts obey the sharing rule, and the sizes.

The rule: tensor A may lie under tensor B only if every op that reads or writes A is a strict ancestor, in the plan's
read-after-write DAG, of every op that writes B -- in the un-grouped plan and with every launch group contracted to one node.  Nothing below
calls the library's own conflict analysis: the DAG is rebuilt here from the `op ... reads ... writes ...` lines of grnet_arena_layout.
"""
import ctypes as C
import random

import pytest

ALIGN = 256                       # bytes: buffers are 256-byte aligned
HEAD = TAIL = 256                 # bytes: the leading zero block, the tail conv_wino4s_f32's masked over-read stays inside
COMPACT = 1                       # GRNET_CREATE_COMPACT_ARENA
PRECISIONS = (0, 1)               # GRNET_PRECISION_F32, GRNET_PRECISION_BF16


def up(x, a=ALIGN):
    return (x + a - 1) // a * a


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def assign(lib, sizes, pairs):
    n = len(sizes)
    sz = (C.c_int64 * max(n, 1))(*sizes)
    flat = [x for p in pairs for x in p]
    pr = (C.c_int32 * max(len(flat), 1))(*flat)
    off = (C.c_int64 * max(n, 1))()
    tot = C.c_int64()
    assert lib.grnet_arena_assign(n, sz, len(pairs), pr, off, C.byref(tot)) == 0
    return list(off)[:n], tot.value


def query(lib, precision, max_frames, flags):
    info = (C.c_int64 * 5)()
    assert lib.grnet_arena_query(precision, max_frames, flags, info) == 0
    return dict(zip(("bytes", "full", "bound", "tensors", "shared"), (int(v) for v in info)))


def layout(lib, precision, max_frames, flags):
    """-> (tensors {id: (name, floats per frame, offset in floats)}, ops [(kind, reads, writes)], groups [[op ...]])"""
    need = lib.grnet_arena_layout(precision, max_frames, flags, None, 0)
    assert need > 0
    buf = C.create_string_buffer(need)
    assert lib.grnet_arena_layout(precision, max_frames, flags, buf, need) == need - 1
    assert lib.grnet_arena_layout(precision, max_frames, flags, buf, need - 1) == -22       # GRNET_EINVAL: too small
    tensors, ops, groups = {}, [], []
    for line in buf.value.decode().splitlines():
        f = line.split()
        if f[0] == "tensor":
            tensors[int(f[1])] = (f[2], int(f[3]), int(f[4]))
        elif f[0] == "op":
            assert int(f[1]) == len(ops) and f[3] == "reads"
            w = f.index("writes")
            ops.append((f[2], [int(x) for x in f[4:w]], [int(x) for x in f[w + 1:]]))
        elif f[0] == "group":
            groups.append([int(x) for x in f[1:]])
        else:
            raise AssertionError("unknown line: " + line)
    return tensors, ops, groups


class Dag:
    """RAW DAG over nodes; node_of maps an op to its node (a contracted group is one node).  Ancestor sets as Python ints (bit i = node i)."""

    def __init__(self, ops, group=()):
        rep = min(group) if group else None
        self.node_of = [rep if i in group else i for i in range(len(ops))]
        n = len(ops)
        deps = [0] * n
        writers = {}
        self.writers, self.touch = {}, {}
        for i, (_, rd, wr) in enumerate(ops):
            me = self.node_of[i]
            for t in rd:
                for w in writers.get(t, ()):
                    if w != me:
                        deps[me] |= 1 << w
            for t in wr:
                writers.setdefault(t, []).append(me)
                self.writers.setdefault(t, set()).add(me)
            for t in rd + wr:
                self.touch.setdefault(t, set()).add(me)
        # strict ancestors by fixpoint (a contracted node's edges do not follow the op order)
        anc = deps[:]
        changed = True
        while changed:
            changed = False
            for i in range(n):
                a, d, k = anc[i], anc[i], 0
                while d:
                    if d & 1:
                        a |= anc[k]
                    d >>= 1
                    k += 1
                if a != anc[i]:
                    anc[i], changed = a, True
        self.anc = anc
        assert all(not (anc[i] >> i) & 1 for i in range(n)), "the contracted plan has a cycle"

    def earlier(self, a, b):
        """every node that touches a is a strict ancestor of every node that writes b"""
        ta, wb = self.touch.get(a), self.writers.get(b)
        if not ta or not wb:
            return False
        return all(x != w and (self.anc[w] >> x) & 1 for x in ta for w in wb)

    def live_across(self, node, t):
        before = any(w == node or (self.anc[node] >> w) & 1 for w in self.writers.get(t, ()))
        after = any(u == node or (self.anc[u] >> node) & 1 for u in self.touch.get(t, ()))
        return before and after


def byte_range(t, max_frames):
    _, per_frame, off = t
    return off * 4, off * 4 + up(per_frame * max_frames * 4)


def overlapping_pairs(tensors, max_frames):
    ids = sorted(tensors)
    rng = {i: byte_range(tensors[i], max_frames) for i in ids}
    return [(a, b) for k, a in enumerate(ids) for b in ids[k + 1:] if rng[a][0] < rng[b][1] and rng[b][0] < rng[a][1]]


# ---------------------------------------------------------------------------------------------------- 1. the assignment
def test_assign_known_graphs(lib):
    sizes = [1000, 70000, 300, 256, 5000]
    off, tot = assign(lib, sizes, [])
    assert tot == up(70000) and off == [0] * 5                                # no conflicts: everything at 0
    pairs = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    off, tot = assign(lib, sizes, pairs)
    assert tot == sum(up(s) for s in sizes)                                   # all pairs conflict: laid end to end
    n = 9
    off, tot = assign(lib, [1000] * n, [(i, i + 1) for i in range(n - 1)])
    assert tot == 2 * up(1000)                                                # a path of equal sizes: two colours
    assert assign(lib, [], []) == ([], 0)
    bad = (C.c_int64 * 1)(-1)
    o, t = (C.c_int64 * 1)(), C.c_int64()
    assert lib.grnet_arena_assign(1, bad, 0, None, o, C.byref(t)) == -22


def test_assign_random_graphs(lib):
    rnd = random.Random(20261017)
    for case in range(300):
        n = rnd.randint(1, 60)
        sizes = [rnd.choice((0, 1, 255, 256, 257, 4096, rnd.randint(1, 1 << 20))) for _ in range(n)]
        p = rnd.choice((0.05, 0.2, 0.5, 0.9))
        pairs = [(a, b) for a in range(n) for b in range(a + 1, n) if rnd.random() < p]
        off, tot = assign(lib, sizes, pairs)
        assert all(o % ALIGN == 0 and o >= 0 for o in off), case
        for a, b in pairs:
            if sizes[a] and sizes[b]:
                assert off[a] + up(sizes[a]) <= off[b] or off[b] + up(sizes[b]) <= off[a], (case, a, b)
        assert tot <= sum(up(s) for s in sizes) and tot >= max(up(s) for s in sizes), case
        assert tot == max(o + up(s) for o, s in zip(off, sizes)), case
        assert assign(lib, sizes, pairs) == (off, tot), case                  # deterministic
        rnd.shuffle(pairs)
        assert assign(lib, sizes, [(b, a) for a, b in pairs]) == (off, tot), case   # ... in the pair list's order and orientation too


# ---------------------------------------------------------------------------------------------------- 2. the real layouts obey the rule
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("max_frames", (16, 400))
def test_compact_layout_obeys_the_sharing_rule(lib, precision, max_frames):
    tensors, ops, groups = layout(lib, precision, max_frames, COMPACT)
    info = query(lib, precision, max_frames, COMPACT)
    assert len(tensors) == info["tensors"] and ops[-1][0] == "COPYOUT"
    total = info["bytes"]
    for t in tensors.values():
        lo, hi = byte_range(t, max_frames)
        assert lo % ALIGN == 0 and lo >= HEAD and hi <= total - TAIL           # aligned, behind the zero block, the tail stays free
    pairs = overlapping_pairs(tensors, max_frames)
    assert len({x for p in pairs for x in p}) == info["shared"] > 0
    forms = [Dag(ops)] + [Dag(ops, set(g)) for g in groups]                     # un-grouped, and every group contracted (building one asserts: no cycle)
    if precision == 1:
        assert len(groups) >= 20                                                # 26 BasicBlock chains, the row walkers, the layer1 pairs
    plain = forms[0]
    for a, b in pairs:
        first, second = (a, b) if plain.earlier(a, b) else (b, a)
        for k, dag in enumerate(forms):
            assert dag.earlier(first, second), f"tensors {tensors[first][0]}#{first} and {tensors[second][0]}#{second} share bytes but form {k} does not order them"
    # what the forward reads after its op list is under nothing: cat, head.heat, head.smpl_feats (the COPYOUT op), head.cam_shape (the POOL op)
    by_name = {v[0]: k for k, v in tensors.items()}
    assert sorted(ops[-1][1]) == sorted(by_name[n] for n in ("cat", "head.heat", "head.smpl_feats"))
    for name in ("cat", "head.heat", "head.smpl_feats", "head.cam_shape"):
        t = by_name[name]
        for a, b in pairs:
            if t in (a, b):
                other = b if a == t else a
                assert plain.earlier(other, t), f"{name} is not the final tenant of its bytes: {tensors[other][0]}#{other} comes later"
    # an op's output never shares bytes with one of its own inputs
    shared = set(pairs)
    for _, rd, wr in ops:
        for r in rd:
            for w in wr:
                assert r == w or (min(r, w), max(r, w)) not in shared


@pytest.mark.parametrize("precision", PRECISIONS)
def test_any_execution_order_reads_what_was_written(lib, precision):
    """The same claim checked by execution instead of by proof: run the plan in seeded random topological orders of its RAW DAG (any lane schedule is
    one), un-grouped and with each launch group as one step, on a model of the compact arena in which a write destroys every other tensor that shares
    bytes with the written one.  No op may read a destroyed or unwritten tensor; a group reads its inputs before AND after its writes (one launch)."""
    max_frames = 64
    tensors, ops, groups = layout(lib, precision, max_frames, COMPACT)
    over = {k: set() for k in tensors}
    for a, b in overlapping_pairs(tensors, max_frames):
        over[a].add(b)
        over[b].add(a)
    rnd = random.Random(7 + precision)
    for group in [()] + [tuple(g) for g in groups] + [()] * 20:
        gset = set(group)
        steps = [[i] for i in range(len(ops)) if i not in gset]
        if group:
            steps.append(list(group))
        node = {i: k for k, st in enumerate(steps) for i in st}
        deps = [set() for _ in steps]
        writers = {}
        for i, (_, rd, wr) in enumerate(ops):
            for t in rd:
                deps[node[i]] |= {w for w in writers.get(t, ()) if w != node[i]}
            for t in wr:
                writers.setdefault(t, set()).add(node[i])
        state = {}                                                               # tensor -> "ok" | "destroyed"
        done, left = set(), set(range(len(steps)))
        while left:
            k = rnd.choice(sorted(x for x in left if deps[x] <= done))
            members = steps[k]
            written = {t for i in members for t in ops[i][2]}
            reads = {t for i in members for t in ops[i][1]} - written            # a group's own intermediates come and go inside the launch
            for t in reads:
                assert state.get(t) == "ok", f"step {members} reads tensor {tensors[t][0]}#{t}: {state.get(t, 'never written')}"
            for t in written:
                for o in over[t]:
                    if o in state:
                        state[o] = "destroyed"
                state[t] = "ok"
            for t in reads:
                assert state.get(t) == "ok", f"step {members} destroys its own input {tensors[t][0]}#{t}"
            done.add(k)
            left.discard(k)
        for t in ops[-1][1]:                                                     # the copy-outs' inputs survive to the end
            assert state[t] == "ok"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_layout_has_no_overlap_and_the_same_plan(lib, precision):
    tensors, ops, groups = layout(lib, precision, 16, 0)
    assert overlapping_pairs(tensors, 16) == []
    ct, cops, cgroups = layout(lib, precision, 16, COMPACT)
    assert cops == ops and cgroups == groups                                    # the plan does not depend on the layout
    assert {k: v[:2] for k, v in ct.items()} == {k: v[:2] for k, v in tensors.items()}
    # today's allocate(): 64 zero floats, then the buffers in creation order, each floats_per_frame * max_frames rounded up to 64 floats
    at = 64
    for k in sorted(tensors):
        assert tensors[k][2] == at
        at += up(tensors[k][1] * 16, 64)
    info = query(lib, precision, 16, 0)
    assert info["bytes"] == info["full"] == (at + 64) * 4 and info["shared"] == 0


# ---------------------------------------------------------------------------------------------------- 3. sizes
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sizes_and_lower_bound(lib, precision):
    for max_frames in (16, 400):
        full, comp = query(lib, precision, max_frames, 0), query(lib, precision, max_frames, COMPACT)
        tensors, ops, groups = layout(lib, precision, max_frames, COMPACT)
        # full bytes = 4 * (64 + sum over tensors of ceil64(floats per frame * max_frames) + 64): grnet::allocate() as it was before layouts existed
        formula = 4 * (64 + sum(up(t[1] * max_frames, 64) for t in tensors.values()) + 64)
        assert full["bytes"] == full["full"] == comp["full"] == formula
        assert comp["bytes"] < full["bytes"]
        # lower bound: the tensors alive across one node (written by it or an ancestor, touched by it or a descendant) conflict pairwise under the
        # rule, so their sum fits in no layout; the largest over every op and over every group contracted alone
        size = {k: up(t[1] * max_frames * 4) for k, t in tensors.items()}
        best = 0
        plain = Dag(ops)
        for node in range(len(ops)):
            best = max(best, sum(size[t] for t in tensors if plain.live_across(node, t)))
        for g in groups:
            dag = Dag(ops, set(g))
            best = max(best, sum(size[t] for t in tensors if dag.live_across(min(g), t)))
        bound = HEAD + best + TAIL
        assert bound == comp["bound"] == full["bound"]
        assert comp["bytes"] >= bound
        print(f"precision {precision} max_frames {max_frames}: full {full['bytes']} compact {comp['bytes']} bound {bound} compact/bound {comp['bytes'] / bound:.3f}")
    if precision == 0:
        assert query(lib, 0, 400, COMPACT)["bytes"] <= 12 * 10**9                  # the bar of the round-6 review (next-step 4): full is 41 GB


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("flags", (0, COMPACT))
def test_sizes_scale_linearly_with_max_frames(lib, precision, flags):
    """A tensor takes ceil64(floats per frame * max_frames) floats.  For max_frames a multiple of 64 nothing is rounded, every size is exactly
    proportional to max_frames, and largest-first first-fit only compares and adds sizes, so scaling every size by k scales every offset by k:
    bytes - head - tail is exactly linear.  For any other max_frames each tensor rounds up by less than 256 bytes, which bounds the full layout."""
    tensors, _, _ = layout(lib, precision, 64, flags)
    var = {m: query(lib, precision, m, flags)["bytes"] - HEAD - TAIL for m in (64, 128, 448, 1024, 2048)}
    assert all(var[m] * 64 == m * var[64] for m in var), var
    t448, _, _ = layout(lib, precision, 448, flags)
    assert all(t448[k][2] - 64 == 7 * (tensors[k][2] - 64) for k in tensors)
    if flags == 0:
        for m in (1, 16, 50, 400):
            got = query(lib, precision, m, 0)["bytes"] - HEAD - TAIL
            assert 0 <= got * 64 - m * var[64] < 64 * ALIGN * len(tensors), m


def test_query_refuses_bad_arguments(lib):
    info = (C.c_int64 * 5)()
    assert lib.grnet_arena_query(0, 0, 0, info) == -22
    assert lib.grnet_arena_query(0, 2049, 0, info) == -22
    assert lib.grnet_arena_query(2, 16, 0, info) == -22
    assert lib.grnet_arena_query(0, 16, 2, info) == -22                          # unknown flag
    assert lib.grnet_arena_query(0, 16, 0, None) == -22
    assert lib.grnet_arena_layout(0, 16, 4, None, 0) == -22
    h = C.c_void_p()
    assert lib.grnet_create_ex(C.byref(h), 0, 0, 16, 2) == -22 and not h.value   # refused before any device is looked at


def test_python_arena_query(pkg, lib):
    q = pkg.arena_query("f32", 400, compact=True)
    assert q["bytes"] == query(lib, 0, 400, COMPACT)["bytes"] and q["full_bytes"] == query(lib, 0, 400, 0)["bytes"]
    assert pkg.arena_query("bf16", 64)["shared_tensors"] == 0
    with pytest.raises(ValueError):
        pkg.arena_query("f16", 64)
    assert pkg.arena_layout("f32", 16, compact=True).startswith("tensor 0 ")
