"""Crafted pair tables for the persistent kernels' lone-wave cone walk (lean_walk_sub64, smm.jl_amd/csrc/smm_walk_lean.hpp), and a plain
restatement of what the exchange plan makes of a pair list (k_exch_plan's cones, smm_cone.hpp): no device, no library.

A pair table is (T, K, 2) int32 with K = N distinct pairs (i, j), i < j, 0-based, as common.random_tables makes them; the crafted list is
the same in every iteration.  exchangeMoves! (AlgoBGP.jl:647-716) walks the list in order, so
    level(pair)  = 1 + max(level of the previous pair of i, level of the previous pair of j)      (no previous pair: 0)
    cone(tile)   = the closure over those predecessors, from the LAST pair of each of the tile's chains
    sub-levels   = sum over the cone's levels of ceil(width / 64)                                 (a sub-level: at most 64 pairs)
    gathered     = the chains the cone's pairs name that are not the tile's own
A cone stays in the persistent form while it has at most CONE_LEVELS sub-levels and CONE_GCAP gathered chains."""
import numpy as np

CONE_LEVELS = 32    # smm_params.hpp
CONE_GCAP = 512
LV_MAXLEV = 31      # levels of a whole pair list the lean plans hold: a deeper injected list keeps the per-iteration kernels
SUB = 64            # pairs per sub-level


# ---- the restatement --------------------------------------------------------------------------------------------------------
def levels(pairs):
    """level of every pair of one list [(i, j), ...] and the two predecessors' positions (-1: none)"""
    last = {}
    lev, pred = [], []
    for k, (i, j) in enumerate(pairs):
        pi, pj = last.get(int(i), -1), last.get(int(j), -1)
        lev.append(1 + max(lev[pi] if pi >= 0 else 0, lev[pj] if pj >= 0 else 0))
        pred.append((pi, pj))
        last[int(i)] = k
        last[int(j)] = k
    return lev, pred, last


def cones(pairs, N, ct):
    """per tile of ct chains: dict(widths=[pairs at level 1, 2, ...], nsub, gathered, fits)"""
    lev, pred, last = levels(pairs)
    out = []
    for c0 in range(0, N, ct):
        own = range(c0, min(c0 + ct, N))
        todo = [last[c] for c in own if c in last]
        seen = set()
        while todo:
            k = todo.pop()
            if k < 0 or k in seen:
                continue
            seen.add(k)
            todo.extend(pred[k])
        depth = max((lev[k] for k in seen), default=0)
        widths = [sum(1 for k in seen if lev[k] == l) for l in range(1, depth + 1)]
        chains = {int(x) for k in seen for x in pairs[k]} - set(own)
        nsub = sum(-(-w // SUB) for w in widths)
        out.append(dict(widths=widths, nsub=nsub, gathered=len(chains), fits=nsub <= CONE_LEVELS and len(chains) <= CONE_GCAP))
    return out


def check_table(tab, N):
    """a pair table as the library takes it: K = N distinct pairs i < j per iteration"""
    assert tab.dtype == np.int32 and tab.ndim == 3 and tab.shape[1:] == (N, 2), tab.shape
    for t in range(tab.shape[0]):
        p = tab[t]
        assert (p[:, 0] < p[:, 1]).all() and p.min() >= 0 and p.max() < N
        assert len({(int(a), int(b)) for a, b in p}) == N, "pairs repeat"


# ---- the generators ---------------------------------------------------------------------------------------------------------
def filler(chains, count):
    """`count` distinct pairs among an even number of chains, in rounds of disjoint pairs: round 0 joins neighbours (2k, 2k + 1), round 1
    (2k + 1, 2k + 2), round r >= 2 (2k, 2k + 2r - 1) — every round is one level deeper than the one before, nothing repeats"""
    L = list(chains)
    M = len(L)
    assert M % 2 == 0 and M >= 8
    out = []
    r = 0
    while len(out) < count:
        s = 1 if r < 2 else 2 * r - 1
        assert s < M - 1, "not enough chains for %d filler pairs" % count
        for k in range(M // 2):
            a = L[(2 * k + (1 if r == 1 else 0)) % M]
            b = L[(2 * k + (1 if r == 1 else 0) + s) % M]
            out.append((min(a, b), max(a, b)))
        r += 1
    return out[:count]


def as_table(pairs, T):
    return np.repeat(np.asarray(pairs, np.int32)[None], T, axis=0)


def chain_table(d, N=80, T=12, ct=16, skip_tiles=0):
    """the dependent chain (0,1), (1,2), ..., (d-1,d): chain d's last pair lies d levels deep — the tile that owns chain d walks exactly d
    sub-levels.  The other N - d pairs are filler among the chains of the tiles BEHIND that tile (skip_tiles: and further that many tiles
    are left out of every pair — nsub = 0 beside tiles that walk), at most a few levels deep."""
    first = (d // ct + 1 + skip_tiles) * ct
    pairs = [(k, k + 1) for k in range(d)] + filler(range(first, N), N - d)
    return as_table(pairs, T)


def tree_table(extra=False, tail=0, N=320, T=12):
    """a binary in-tree into tile 0: 128 disjoint leaf pairs at level 1 (chains 0..255), joined pairwise through one endpoint each at the
    levels 2, 3, 4 into 16 pairs, each of which ends in one chain of tile 0 (chains 0..15): the cone of tile 0 has the widths
    128 / 64 / 32 / 16 — two sub-levels of one level, then whole and part sub-levels — and gathers 240 chains.
    extra: one more pair at level 2 on four chains of their own, joined to tile 0's chain 15 at the levels 3 and 5: widths
    130 / 65 / 33 / 16 / 1 (a level one pair past a sub-level), 244 gathered chains.
    tail: that many further pairs (15, a), each with a chain of its own, behind chain 15's last pair — one level and one sub-level each:
    the way to the cap of 32 sub-levels, and past it, for a list that is no more than 31 levels deep."""
    lv = [[], [], [], [], []]
    for q in range(16):
        c = [q] + list(range(16 + 15 * q, 31 + 15 * q))          # the root's 16 chains: x = c[0] in tile 0
        lv[0] += [(c[2 * k], c[2 * k + 1]) for k in range(8)]      # leaves (c0,c1) (c2,c3) ... (c14,c15)
        lv[1] += [(c[4 * k], c[4 * k + 2]) for k in range(4)]      # (c0,c2) (c4,c6) (c8,c10) (c12,c14)
        lv[2] += [(c[0], c[4]), (c[8], c[12])]
        lv[3] += [(c[0], c[8])]
    used = 256
    if extra:
        e = [256, 257, 258, 259]
        lv[0] += [(e[0], e[1]), (e[2], e[3])]
        lv[1] += [(e[0], e[2])]
        lv[2] += [(255, e[0])]           # chain 255: root 15's last leaf chain, in no pair past level 1
        lv[4] += [(15, e[0])]            # behind chain 15's level-4 pair
        used = 260
    pairs = [(min(a, b), max(a, b)) for l in lv for (a, b) in l]
    pairs += [(15, used + k) for k in range(tail)]
    used += tail + (used + tail) % 2
    pairs += filler(range(used, N), N - len(pairs))
    return as_table(pairs, T)


# what the GPU test says of its tables, for tests/test_cone_craft.py to hold against the restatement:
# name -> (table, N, ct, {tile: (nsub, widths or None, gathered or None)}, every cone fits)
def claims():
    out = {}
    for d in (1, 2, 3, 4, 5, 6, 7, 31, 32, 33):
        own = d // 16
        want = {own: (d, [1] * d if own == 0 else None, None)}
        out["chain%d" % d] = (chain_table(d), 80, 16, want, d <= CONE_LEVELS)
    out["chain3_idle_tile"] = (chain_table(3, skip_tiles=1), 80, 16, {0: (3, [1, 1, 1], 0), 1: (0, [], 0)}, True)
    out["tree"] = (tree_table(), 320, 16, {0: (5, [128, 64, 32, 16], 240)}, True)
    out["tree_extra"] = (tree_table(extra=True), 320, 16, {0: (8, [130, 65, 33, 16, 1], 244)}, True)
    out["tree_cap32"] = (tree_table(tail=27), 320, 16, {0: (32, [128, 64, 32, 16] + [1] * 27, 267)}, True)
    out["tree_past33"] = (tree_table(extra=True, tail=25), 320, 16, {0: (33, [130, 65, 33, 16, 1] + [1] * 25, 269)}, False)
    # the forms on tiles of 32 chains (k_chain_persist_gen): the same lists, N = 96
    for d in (3, 31):
        out["chain%d_ct32" % d] = (chain_table(d, N=96, ct=32), 96, 32, {d // 32: (d, None, None)}, True)
    return out
