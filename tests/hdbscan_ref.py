"""Reference for csrc/mst.hip and clip/hdbscan.py: float64 and plain numpy, needs no library.

Two kinds of check.
  float64   mutual reachability from the 16-bit rows, Prim's tree, the bottleneck ("path max" for distances; for similarities
            the path MIN) matrix of a tree, and `check_mst`: the edges form a spanning tree and no pair outside the tree is
            closer than the weakest edge on the tree path between its rows, within a tolerance.  The device decides on fp32
            values that lie within the pair tolerance `tol` of the float64 ones (a core value is an order statistic of such
            values, so it does too).  err = the largest excess of a pair outside the tree over its path's weakest edge, in
            float64; err <= tol is asserted and err / tol is the figure reported.  (Both the pair and the path edge can move
            by tol, so 2 tol is what the argument allows in the worst case; the bound asserted is the stricter one, the pair
            tolerance itself, which already carries a factor 4 over the rounding of a sequential sum.)
  exact     `exact_mst`: Kruskal under the strict total order (larger m, then smaller min(i, j), then smaller max(i, j)) on
            given fp32 score bits - the device's own.  The tree under that order is unique: the comparison has no tolerance.
Then an independent condensed tree (sets and recursion, where clip/hdbscan.py keeps arrays and stacks), and `boruvka_np`, a
restatement of the device rounds with the planted faults the tests must see caught.
"""
import itertools

import numpy as np

MASK = 0xFFFFFFFF
FAULTS = ("mask", "no_core_j", "tie_high", "m_only", "stale")


# ---- keys -----------------------------------------------------------------------------------------------------------------
def score_keys(v):
    """the kernels' score_key on an fp32 array: uint64 values below 2^32; -0 == +0, NaN -> 0"""
    v = np.asarray(v, dtype=np.float32) + np.float32(0.0)
    b = v.view(np.uint32).astype(np.uint64)
    neg = (b & 0x80000000) != 0
    k = np.where(neg, ~b & MASK, b | 0x80000000)
    return np.where(np.isnan(v), np.uint64(0), k).astype(np.uint64)


def key_values(k):
    """the fp32 value of score keys (0 -> NaN)"""
    k = np.asarray(k, dtype=np.uint64)
    b = np.where(k & 0x80000000 != 0, k ^ 0x80000000, ~k & MASK).astype(np.uint32)
    out = b.view(np.float32).copy()
    out[k == 0] = np.nan
    return out


def mreach_keys(S_bits, core, drop_core_j=False):
    """uint64 [N, N]: the key of m[i, j] = min(s, core_i, core_j) from fp32 score bits and fp32 core values"""
    ks, kc = score_keys(S_bits), score_keys(core)
    mk = np.minimum(ks, kc[:, None])
    return mk if drop_core_j else np.minimum(mk, kc[None, :])


def nearest_keys(S_bits, core, comp, fault=None):
    """what cclip_mreach_nearest returns, from the same bits: uint64 [N]"""
    N = len(core)
    mk = mreach_keys(S_bits, core, drop_core_j=fault == "no_core_j")
    comp = np.asarray(comp)
    valid = ~np.eye(N, dtype=bool) if fault == "mask" else comp[None, :] != comp[:, None]
    j = np.arange(N, dtype=np.uint64)
    low = j if fault == "tie_high" else (~j & MASK)
    key = (mk << np.uint64(32)) | low[None, :]
    key = np.where(valid, key, np.uint64(0)).max(axis=1) if N else np.zeros(0, np.uint64)
    if fault == "tie_high":                                # back to the ~j form
        key = np.where(key == 0, key, (key & ~np.uint64(MASK)) | (~key & MASK))
    return key


# ---- float64 ----------------------------------------------------------------------------------------------------------------
def scores64(x16):
    x = x16.double().numpy()
    return x @ x.T


def core64(S, min_samples):
    """the min_samples-th largest entry of every row, the row itself counted; +inf for 1"""
    if min_samples == 1:
        return np.full(S.shape[0], np.inf)
    return -np.sort(-S, axis=1)[:, min_samples - 1]


def mreach64(S, core):
    return np.minimum(np.minimum(S, core[:, None]), core[None, :])


def chord64(m):
    return np.sqrt(np.maximum(0.0, 2.0 - 2.0 * np.asarray(m, dtype=np.float64)))


def prim(M):
    """Prim's MAXIMUM spanning tree of the symmetric weights M: (edges [(i, j)], total weight)"""
    N = M.shape[0]
    inside = np.zeros(N, dtype=bool)
    inside[0] = True
    best, frm = M[0].copy(), np.zeros(N, dtype=np.int64)
    edges, total = [], 0.0
    for _ in range(N - 1):
        cand = np.where(inside, -np.inf, best)
        j = int(np.argmax(cand))
        edges.append((int(frm[j]), j))
        total += float(M[frm[j], j])
        inside[j] = True
        better = M[j] > best
        best, frm = np.where(better, M[j], best), np.where(better, j, frm)
    return edges, total


def is_spanning_tree(N, u, v):
    if len(u) != N - 1:
        return False
    parent = list(range(N))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(u, v):
        a, b = int(a), int(b)
        if not (0 <= a < N and 0 <= b < N) or a == b:
            return False
        ra, rb = find(a), find(b)
        if ra == rb:
            return False
        parent[ra] = rb
    return True


def path_weakest(N, u, v, w):
    """[N, N]: the weakest (smallest) weight on the tree path between every two rows, by union-find over the edges from the
    strongest down - the edge that first joins two groups is the weakest on every path between them"""
    B = np.full((N, N), np.inf)
    members = {i: [i] for i in range(N)}
    head = list(range(N))
    for k in np.argsort(-np.asarray(w, dtype=np.float64), kind="stable"):
        a, b = head[int(u[k])], head[int(v[k])]
        A, Bm = members[a], members[b]
        B[np.ix_(A, Bm)] = w[k]
        B[np.ix_(Bm, A)] = w[k]
        if len(A) < len(Bm):
            a, b, A, Bm = b, a, Bm, A
        A.extend(Bm)
        for r in Bm:
            head[r] = a
        del members[b]
    return B


def check_mst(u, v, M, tol):
    """(ok, err / tol): the edges are a spanning tree of the N rows, and every pair outside the tree is at most tol better than
    the weakest edge (weights from M) on the tree path between its rows"""
    N = M.shape[0]
    if not is_spanning_tree(N, u, v):
        return False, np.inf
    if N < 3:
        return True, 0.0
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    weakest = path_weakest(N, u, v, M[u, v])
    excess = M - weakest
    np.fill_diagonal(excess, -np.inf)
    excess[u, v] = excess[v, u] = -np.inf
    err = max(float(excess.max()), 0.0)
    return err <= tol, err / tol


# ---- exact ------------------------------------------------------------------------------------------------------------------
def sorted_pairs(mk):
    """every pair i < j in the total order: (i, j, key) arrays, best edge first"""
    N = mk.shape[0]
    i, j = np.triu_indices(N, 1)
    k = mk[i, j]
    if N < 65536:
        order = np.argsort(((MASK - k) << np.uint64(32)) | (i.astype(np.uint64) << np.uint64(16)) | j.astype(np.uint64), kind="stable")
    else:
        order = np.lexsort((j, i, MASK - k))
    return i[order], j[order], k[order]


def kruskal(N, i, j):
    """indices into the sorted pair list of the N - 1 edges Kruskal keeps.  Blocks of pairs are filtered with the labels as
    they stood at the block's start (a pair inside one component then can never be kept), the rest is the plain loop."""
    parent = np.arange(N)

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    kept, block, at = [], 4096, 0
    while len(kept) < N - 1 and at < len(i):
        lab = np.array([find(a) for a in range(N)])
        sel = np.nonzero(lab[i[at:at + block]] != lab[j[at:at + block]])[0] + at
        for e in sel:
            ra, rb = find(int(i[e])), find(int(j[e]))
            if ra != rb:
                parent[ra] = rb
                kept.append(int(e))
        at += block
        block *= 2
    return kept


def exact_mst(S_bits, core, drop_core_j=False):
    """the unique maximum spanning tree under the total order on the given bits: a set of (i, j, key) with i < j"""
    mk = mreach_keys(S_bits, core, drop_core_j)
    N = mk.shape[0]
    i, j, k = sorted_pairs(mk)
    return {(int(i[e]), int(j[e]), int(k[e])) for e in kruskal(N, i, j)}


def brute_force_mst(S_bits, core):
    """the best spanning tree by enumeration (N <= 7): with a strict order on edges the best tree is the one whose sorted
    ranks come first lexicographically, and combinations() lists the rank tuples in that very order"""
    mk = mreach_keys(S_bits, core)
    N = mk.shape[0]
    i, j, k = sorted_pairs(mk)
    for pick in itertools.combinations(range(len(i)), N - 1):
        if is_spanning_tree(N, i[list(pick)], j[list(pick)]):
            return {(int(i[e]), int(j[e]), int(k[e])) for e in pick}
    return None


def edge_set(u, v, m):
    """device slots -> the set of (i, j, key) with i < j; empty slots (u < 0) dropped"""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    k = score_keys(m)
    return {(int(min(a, b)), int(max(a, b)), int(kk)) for a, b, kk in zip(u, v, k) if a >= 0}


def sort_edges(edges):
    """a set of (i, j, key) -> (u, v, m fp32) arrays in the total order"""
    e = sorted(edges, key=lambda t: (-t[2], t[0], t[1]))
    u = np.array([t[0] for t in e], dtype=np.int64)
    v = np.array([t[1] for t in e], dtype=np.int64)
    return u, v, key_values(np.array([t[2] for t in e], dtype=np.uint64))


# ---- the device rounds, restated, with planted faults -------------------------------------------------------------------------
def boruvka_np(S_bits, core, fault=None):
    """(u, v, m) slot arrays as cclip_mst_boruvka fills them.  Faults: "mask" the nearest search ignores comp (only j != i);
    "no_core_j" m = min(s, core_i); "tie_high" equal m goes to the higher j; "m_only" the component reduction compares by m
    alone; "stale" the nearest search reads the labels of the round before."""
    N = len(core)
    u, v = np.full(N, -1, dtype=np.int64), np.full(N, -1, dtype=np.int64)
    m = np.full(N, np.nan, dtype=np.float32)
    comp, prev = np.arange(N), np.arange(N)
    rounds = int(np.ceil(np.log2(N))) if N > 1 else 0
    for _ in range(rounds):
        if len(set(comp.tolist())) == 1:
            break
        keys = nearest_keys(S_bits, core, prev if fault == "stale" else comp, fault)
        best = {}
        for i in range(N):
            if keys[i] == 0:
                continue
            j = int(~keys[i] & MASK)
            cand = (int(keys[i] >> np.uint64(32)), -min(i, j), -max(i, j))
            c = int(comp[i])
            if c not in best or (cand[0] >= best[c][0] if fault == "m_only" else cand > best[c]):
                best[c] = cand
        parent = np.arange(N)
        for c, (k, lo, hi) in best.items():
            lo, hi = -lo, -hi
            i, j = (lo, hi) if comp[lo] == c else (hi, lo)
            t = int(comp[j])
            same = best.get(t) == (k, -lo, -hi)
            if t != c and not (same and c < t):
                parent[c] = t
                u[c], v[c], m[c] = i, j, key_values([k])[0]
        new = comp.copy()
        for i in range(N):
            r = int(comp[i])
            for _step in range(N):
                if parent[r] == r:
                    break
                r = int(parent[r])
            new[i] = r
        prev, comp = comp, new
    return u, v, m


def swap_heavier(edges, mk):
    """a tree with one edge replaced by a strictly weaker pair that still spans: None if the set has none"""
    N = mk.shape[0]
    e = sorted(edges)
    for a in range(len(e)):
        rest = e[:a] + e[a + 1:]
        for i in range(N):
            for j in range(i + 1, N):
                if int(mk[i, j]) < e[a][2] and is_spanning_tree(N, [t[0] for t in rest] + [i], [t[1] for t in rest] + [j]):
                    return set(rest) | {(i, j, int(mk[i, j]))}
    return None


# ---- the condensed tree, independently: sets and recursion ---------------------------------------------------------------------
def ref_clusters(n, u, v, d, min_cluster_size, method="eom", allow_single_cluster=False, lam_of=None):
    """(labels, probabilities) from tree edges in merge order with distances d.  lam_of: distance -> lambda, default
    1 / max(d, 1e-6) (the planted fault passes another)."""
    lam_of = lam_of or (lambda dist: 1.0 / max(dist, 1e-6))
    labels, prob = np.full(n, -1, dtype=np.int64), np.zeros(n)
    if n == 1:
        if allow_single_cluster:
            labels[0], prob[0] = 0, 1.0
        return labels, prob
    node_of = {p: ("leaf", frozenset([p])) for p in range(n)}
    top = None
    for k in range(n - 1):
        a, b = node_of[int(u[k])], node_of[int(v[k])]
        assert a is not b, "the edges are no spanning tree"
        top = ("split", a[1] | b[1], lam_of(float(d[k])), a, b)
        for p in top[1]:
            node_of[p] = top

    clusters = []                                          # dicts: birth, falls [(point, lambda)], kids [index]

    def grow(node, cid):
        """follow cluster cid down from `node`"""
        while node[0] == "split":
            _, _, lam, a, b = node
            big = [s for s in (a, b) if len(s[1]) >= min_cluster_size]
            if len(big) == 2:
                for s in (a, b):
                    clusters.append({"birth": lam, "falls": [], "kids": [], "size": len(s[1])})
                    clusters[cid]["kids"].append(len(clusters) - 1)
                    grow(s, len(clusters) - 1)
                return
            for s in (a, b):
                if s not in big:
                    clusters[cid]["falls"].extend((p, lam) for p in sorted(s[1]))
            if not big:
                return
            node = big[0]

    clusters.append({"birth": 0.0, "falls": [], "kids": [], "size": n})
    grow(top, 0)

    def stability(c):
        cl = clusters[c]
        return sum(lam - cl["birth"] for _, lam in cl["falls"]) + sum(
            (clusters[k]["birth"] - cl["birth"]) * clusters[k]["size"] for k in cl["kids"])

    def eom(c, allowed):
        below, chosen = 0.0, []
        for k in clusters[c]["kids"]:
            s, ch = eom(k, True)
            below += s
            chosen += ch
        own = stability(c)
        if allowed and not below > own:
            return own, [c]
        return below, chosen

    def leaves(c):
        kids = clusters[c]["kids"]
        return [c] if not kids else [x for k in kids for x in leaves(k)]

    if method == "eom":
        chosen = eom(0, allow_single_cluster)[1]
    else:
        chosen = leaves(0)
        if chosen == [0] and not allow_single_cluster:
            chosen = []

    def points(c):
        out = list(clusters[c]["falls"])
        for k in clusters[c]["kids"]:
            out += points(k)
        return out

    groups = []
    for c in chosen:
        cl = clusters[c]
        lam_max = max([lam for _, lam in cl["falls"]] + [clusters[k]["birth"] for k in cl["kids"]])
        pts = points(c)
        groups.append((min(p for p, _ in pts), pts, lam_max))
    for number, (_, pts, lam_max) in enumerate(sorted(groups, key=lambda g: g[0])):
        for p, lam in pts:
            labels[p] = number
            prob[p] = min(lam, lam_max) / lam_max
    return labels, prob


# ---- data -------------------------------------------------------------------------------------------------------------------
def unit16(x64, dtype):
    """float64 rows -> normalised, rounded to the 16-bit torch dtype"""
    import torch
    x = np.asarray(x64, dtype=np.float64)
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return torch.from_numpy(x).to(torch.float32).to(dtype)


def planted_recipe(dtype):
    """default_rng(0): 4 unit centres in D = 32, 40 rows each at centre + 0.08 randn, 12 rows of pure randn; normalised and
    rounded.  Returns (x16 [172, 32], planted labels with -1 for the 12 noise rows)."""
    rng = np.random.default_rng(0)
    centres = rng.standard_normal((4, 32))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    rows = [centres[c] + 0.08 * rng.standard_normal((40, 32)) for c in range(4)]
    rows.append(rng.standard_normal((12, 32)))
    labels = np.repeat(np.arange(5), [40, 40, 40, 40, 12])
    labels[labels == 4] = -1
    return unit16(np.concatenate(rows), dtype), labels


def random_rows(N, D, seed, dtype, dup_fraction=0.0):
    """random unit rows; with dup_fraction, that share of the rows are bitwise copies of earlier rows"""
    rng = np.random.default_rng(seed)
    x = unit16(rng.standard_normal((N, D)), dtype)
    ndup = int(N * dup_fraction)
    if ndup:
        dst = rng.choice(np.arange(1, N), size=min(ndup, N - 1), replace=False)
        for t in dst:
            x[int(t)] = x[int(rng.integers(0, t))]
    return x


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def adjusted_rand(a, b):
    a, b = np.asarray(a), np.asarray(b)
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    table = np.zeros((len(ua), len(ub)))
    np.add.at(table, (ia, ib), 1)
    comb = lambda x: x * (x - 1) / 2.0
    s, ra, rb, n = comb(table).sum(), comb(table.sum(1)).sum(), comb(table.sum(0)).sum(), comb(len(a))
    expected = ra * rb / n
    return (s - expected) / (0.5 * (ra + rb) - expected)
