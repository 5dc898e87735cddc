"""float64 reference of k-centre greedy selection on the same 16-bit operands (csrc/coreset.hip, clip/coreset.py), the bounds
its tests use, an fp32 restatement of the kernel in the kernel's own order with planted faults, and the brute-force optimum
for tiny N.  numpy on the host; needs no library.

Tolerances (derived, none measured; u = 2^-24, the unit roundoff of fp32).  Products of two bf16 or two fp16 values are exact
in fp32, so a distance d = 1 - s carries only the summation error of s - at most (D - 1) u sum_k |x_ik x_ck| to first order
for ANY order of the D - 1 additions (the kernel's longest chain is 7 + 1 + 6 additions, far below D - 1) - and the rounding of
the subtraction:

    tol_d(i, c) = (D - 1) u sum_k |x_ik x_ck| + u |1 - s|

mind[i] is a minimum of such distances and a minimum is 1-Lipschitz in every argument, so mind[i] carries the largest tol_d
among the centres the row has met; a weighted key w d adds one more rounding, u w d.
Seeding goes through cclip_kmeans_assign, whose score is an MFMA chain: tests/kmeans_ref.py allows a factor 4 on the summation
term for the MFMA's internal order, and so does seed_tol here; clamp(1 - best, min = 0) is 1-Lipschitz again.

A selection is correct when the float64 key of the device's pick is within tol(pick) + tol(arg-max) of the float64 maximum,
replayed from the device's OWN earlier picks: every pick is checked, none left out, and the replay cannot diverge after a
near-tie.  An owner is correct when its float64 distance is within tolerance of the row's minimum.  Where the kernel's order is
exact - bitwise equal rows give bitwise equal keys and distances - the rules are checked exactly: the lower row wins, the
earlier centre keeps the row.
"""
import itertools

import numpy as np

U = 2.0 ** -24
INF = float("inf")


def rows64(x16):
    """a 16-bit torch tensor [N, D] (any strides) -> float64 numpy"""
    return x16.detach().cpu().double().numpy()


def dist64(X, c):
    return 1.0 - X @ X[c]


def tol_d(X, c, factor=1.0):
    D = X.shape[1]
    return factor * (D - 1) * U * (np.abs(X) @ np.abs(X[c])) + U * np.abs(1.0 - X @ X[c])


def seed_tol(X, c):
    """the bound for a distance that came out of the MFMA assignment kernel (seeding): factor 4 on the summation term"""
    return tol_d(X, c, 4.0)


def eligible(owner, w):
    e = owner != np.arange(owner.shape[0])
    if w is not None:
        with np.errstate(invalid="ignore"):
            e = e & (w > 0)
    return e


def key_values(w, mind):
    if w is None:
        return mind.copy()
    with np.errstate(invalid="ignore"):
        return w * mind


def argmax_key(vals, elig, tie_high=False):
    """the kernel's order: larger first, NaN below every number, equal values to the lower row; -1 if no row is eligible"""
    rows = np.nonzero(elig)[0]
    if rows.size == 0:
        return -1
    v = vals[rows]
    nan = np.isnan(v)
    if nan.all():
        return int(rows[-1] if tie_high else rows[0])
    top = np.max(v[~nan])
    hits = rows[(v == top) & ~nan]
    return int(hits[-1] if tie_high else hits[0])


def new_state(N):
    return dict(mind=np.full(N, INF), owner=np.full(N, -1, dtype=np.int64), tol=np.zeros(N))


def seeded_state(X, seeds):
    """float64 state with the rows `seeds` as centres from the start (the lower seed on equal distance: kmeans_assign's rule)"""
    N = X.shape[0]
    st = new_state(N)
    for c in sorted(int(s) for s in seeds):
        d = dist64(X, c)
        t = seed_tol(X, c)
        st["tol"] = np.maximum(st["tol"], t)
        better = d < st["mind"]
        st["mind"] = np.where(better, d, st["mind"])
        st["owner"] = np.where(better, c, st["owner"])
    st["mind"] = np.maximum(st["mind"], 0.0)
    for c in seeds:
        st["mind"][c], st["owner"][c] = 0.0, c
    return st


def step(X, w, mind, owner, c, tol=None):
    """One update in float64 under the kernel's rules.  Returns (mind, owner, radius, tol): radius = mind[c] before the update;
    a centre keeps its 0; a strictly smaller distance takes the row; a NaN distance changes nothing."""
    N = X.shape[0]
    d = dist64(X, c)
    rows = np.arange(N)
    with np.errstate(invalid="ignore"):
        take = (owner != rows) & (d < mind)
    take[c] = False
    mind2, owner2 = np.where(take, d, mind), np.where(take, c, owner)
    radius = mind[c]
    mind2[c], owner2[c] = 0.0, c
    tol2 = None
    if tol is not None:
        tol2 = np.where(owner != rows, np.maximum(tol, tol_d(X, c)), tol)
        tol2[c] = 0.0
    return mind2, owner2, radius, tol2


def greedy(X, w, m, seeds=(), first=None):
    """float64 k-centre greedy: returns dict(picks, radius, mind, owner, tol, gaps); gaps[t] = best minus second-best eligible key
    at pick t (inf if there is no second, nan for a given first row)"""
    st = seeded_state(X, seeds) if len(seeds) else new_state(X.shape[0])
    mind, owner, tol = st["mind"], st["owner"], st["tol"]
    picks, radius, gaps = [], [], []
    for t in range(m):
        if t == 0 and first is not None:
            c, gap = int(first), float("nan")
        else:
            vals, el = key_values(w, mind), eligible(owner, w)
            c = argmax_key(vals, el)
            if c < 0:
                picks.append(-1); radius.append(float("nan")); gaps.append(float("nan"))
                continue
            rest = el.copy(); rest[c] = False
            with np.errstate(invalid="ignore"):
                gap = vals[c] - np.max(vals[rest]) if rest.any() else INF
        mind, owner, r, tol = step(X, w, mind, owner, c, tol)
        picks.append(c); radius.append(r); gaps.append(gap)
    return dict(picks=np.array(picks, dtype=np.int64), radius=np.array(radius), mind=mind, owner=owner, tol=tol,
                gaps=np.array(gaps))


def numpy_greedy(X, m, first):
    """the plain textbook loop, for the reference to be compared against: unweighted, no seeds"""
    N = X.shape[0]
    mind = np.full(N, INF)
    chosen = []
    c = first
    for _ in range(m):
        chosen.append(c)
        mind = np.minimum(mind, 1.0 - X @ X[c])
        mind[chosen] = -1.0                                 # never again
        c = int(np.argmax(mind))
    mind[chosen] = 0.0
    return np.array(chosen), mind


def optimal_radius(Dm, m):
    """brute force: the smallest covering radius m centres can reach, for a full distance matrix Dm [N, N] (tiny N)"""
    N = Dm.shape[0]
    return min(np.max(np.min(Dm[:, list(cs)], axis=1)) for cs in itertools.combinations(range(N), m))


# ---------------------------------------------------------------------------------------------------------------------------
# the checks


def key_tol(w, mind, tol):
    if w is None:
        return tol
    with np.errstate(invalid="ignore"):
        wd = np.where(np.isfinite(w * mind), np.abs(w * mind), 0.0)
        return np.where(w > 0, np.abs(w) * tol + U * wd, 0.0)


def check_step(X, w, mind0, owner0, c, mind1, owner1, radius1=None):
    """One given-centre update of the device, (mind0, owner0) -> (mind1, owner1), against the float64 step.  Returns (problems,
    largest err / tol)."""
    N = X.shape[0]
    rows = np.arange(N)
    mref, oref, rref, _ = step(X, w, mind0.astype(np.float64), owner0.astype(np.int64), c)
    tol = tol_d(X, c)
    d = dist64(X, c)
    bad, worst = [], 0.0
    both_inf = np.isinf(mref) & (mind1 == mref)
    with np.errstate(invalid="ignore"):
        err = np.where(both_inf, 0.0, np.abs(mind1 - mref))
    fixed = (owner0 == rows) | (rows == c)                   # exact: a centre keeps its state, row c becomes 0 / c
    if not np.array_equal(mind1[fixed], mref[fixed]) or not np.array_equal(owner1[fixed], oref[fixed]):
        bad.append("a centre row (or row c) does not hold its exact state")
    free = ~fixed
    if free.any():
        ratio = err[free] / tol[free]
        worst = float(np.nanmax(ratio)) if ratio.size else 0.0
        if not (err[free] <= tol[free]).all():
            bad.append(f"mind off by {worst:.3g} tol at row {int(rows[free][np.nanargmax(ratio)])}")
        took = owner1[free] == c
        kept = owner1[free] == owner0[free]
        if not (took | kept).all():
            bad.append("an owner that is neither the old one nor c")
        with np.errstate(invalid="ignore"):
            if not (d[free][took & ~kept] <= mind0[free][took & ~kept] + tol[free][took & ~kept]).all():
                bad.append("a row went to c although c is farther than its old centre")
            if not (d[free][kept & ~took] >= mind0[free][kept & ~took] - tol[free][kept & ~took]).all():
                bad.append("a row kept its centre although c is nearer")
        # mind and owner move together
        moved = mind1[free] != mind0[free]
        if (moved & ~took).any():
            bad.append("mind changed without the owner becoming c")
    if radius1 is not None:
        r0 = mind0[c]
        if not (radius1 == r0 or (np.isnan(radius1) and np.isnan(r0))):
            bad.append(f"radius {radius1} is not mind[c] before the update ({r0})")
    return bad, worst


def check_selection(X, w, picks, radius, mind_dev, owner_dev, seeds=(), first=None):
    """Replay the device's own picks in float64.  Returns (problems, largest err / tol over keys, radii, distances and owners)."""
    N = X.shape[0]
    rows = np.arange(N)
    st = seeded_state(X, seeds) if len(seeds) else new_state(N)
    mind, owner, tol = st["mind"], st["owner"], st["tol"]
    order = {int(s): -1 for s in seeds}                      # centre -> when it became one
    bad, worst = [], 0.0
    for t, p in enumerate(int(v) for v in picks):
        vals, el = key_values(w, mind), eligible(owner, w)
        kt = key_tol(w, mind, tol)
        if p < 0:
            if el.any():
                bad.append(f"pick {t}: -1 although row {int(np.nonzero(el)[0][0])} is eligible")
            if not np.isnan(radius[t]):
                bad.append(f"pick {t}: radius {radius[t]} with pick -1")
            continue
        if p >= N or not el[p]:
            why = "a centre" if p < N and owner[p] == p else "not eligible (weight)"
            bad.append(f"pick {t}: row {p} is {why}")
            if p >= N:
                continue
        if not (t == 0 and first is not None):
            best = argmax_key(vals, el)
            if best >= 0 and not np.isnan(vals[best]):
                slack = kt[p] + kt[best]
                if not vals[p] + slack >= vals[best]:
                    bad.append(f"pick {t}: row {p} key {vals[p]:.9g} below the maximum {vals[best]:.9g} (row {best}) by more than {slack:.3g}")
                elif np.isfinite(vals[best]) and slack > 0:
                    worst = max(worst, float((vals[best] - vals[p]) / slack))
                # exact where the kernel is exact: a bitwise equal lower row with the same weight carries the same key
                twins = np.nonzero(el[:p] & np.all(X[:p] == X[p], axis=1) & (mind[:p] == mind[p]))[0]
                if w is not None:
                    twins = twins[w[twins] == w[p]]
                if twins.size:
                    bad.append(f"pick {t}: row {p} chosen although its equal row {int(twins[0])} is lower")
        elif p != first:
            bad.append(f"pick 0: row {p}, not the given first row {first}")
        r_ok = (np.isinf(mind[p]) and radius[t] == mind[p]) or abs(radius[t] - mind[p]) <= tol[p]
        if not r_ok:
            bad.append(f"pick {t}: radius {radius[t]:.9g} against mind[pick] {mind[p]:.9g} before the update (tol {tol[p]:.3g})")
        elif np.isfinite(mind[p]) and tol[p] > 0:
            worst = max(worst, float(abs(radius[t] - mind[p]) / tol[p]))
        mind, owner, _, tol = step(X, w, mind, owner, p, tol)
        order[p] = t
    # the final state: every distance and every owner, no row left out
    cents = np.array(sorted(order), dtype=np.int64)
    if cents.size == 0:
        if not (np.isinf(mind_dev).all() and (owner_dev == -1).all()):
            bad.append("state changed without a centre")
        return bad, worst
    is_c = np.zeros(N, dtype=bool); is_c[cents] = True
    if not ((mind_dev[is_c] == 0).all() and (owner_dev[is_c] == rows[is_c]).all()):
        bad.append("a centre without distance 0 / owner itself")
    with np.errstate(invalid="ignore"):
        err = np.abs(mind_dev - mind)
    free = ~is_c
    if free.any():
        ratio = np.where(tol[free] > 0, err[free] / np.where(tol[free] > 0, tol[free], 1.0), np.where(err[free] > 0, INF, 0.0))
        worst = max(worst, float(ratio.max()))
        if not (err[free] <= tol[free]).all():
            i = int(rows[free][np.argmax(ratio)])
            bad.append(f"distance of row {i}: {mind_dev[i]:.9g} against {mind[i]:.9g} ({ratio.max():.3g} tol)")
        od = owner_dev[free]
        if not np.isin(od, cents).all():
            bad.append("an owner that is no centre")
        else:
            down = 1.0 - np.einsum("ij,ij->i", X[free], X[od])
            if not (down <= mind[free] + tol[free]).all():
                i = int(rows[free][np.argmax(down - mind[free] - tol[free])])
                bad.append(f"owner of row {i} is farther than the row's nearest centre by more than the tolerance")
            # exact where the kernel is exact: of bitwise equal centre rows the one chosen first keeps the row (among picks; among
            # seeds the lowest row, the assignment kernel's rule; a seed and a pick come from two kernels and are not compared)
            when = np.array([order[int(c)] for c in cents])
            for i, o in zip(rows[free], od):
                grp = np.all(X[cents] == X[o], axis=1)
                same, wh = cents[grp], when[grp]
                if same.size > 1 and ((wh >= 0).all() or (wh < 0).all()):
                    first_c = same[np.argmin(wh)]
                    if o != first_c:
                        bad.append(f"row {int(i)} went to centre {int(o)}, a later copy of centre {int(first_c)}")
                        break
    return bad, worst


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel restated in fp32, in its own order, with one planted fault at a time

FAULTS = ("tie_high", "centre_eligible", "overwrite", "owner_le", "weight_ignored", "radius_after", "stale_partials",
          "rows_skipped", "nan_weight")


def team_lanes(D):
    t = 4
    while t * 8 < min(D, 512):
        t *= 2
    return t


def dot32(X32, c32):
    """fp32 <x_i, c> in the kernel's order: per lane 8 products added ascending, the second pass (D > 512) likewise and added,
    then the team's xor butterfly over lane distances 1, 2, .. T / 2"""
    N, D = X32.shape
    T = team_lanes(D)
    prod = (X32 * c32[None, :]).astype(np.float32)          # exact: 16-bit operands

    def lanes(block):
        pad = np.zeros((N, T * 8), dtype=np.float32)
        pad[:, :block.shape[1]] = block
        p = pad.reshape(N, T, 8)
        acc = p[:, :, 0].copy()
        for j in range(1, 8):
            acc = (acc + p[:, :, j]).astype(np.float32)
        return acc

    acc = lanes(prod[:, :512])
    if D > 512:
        acc = (acc + lanes(prod[:, 512:])).astype(np.float32)
    lane = np.arange(T)
    d = 1
    while d < T:
        acc = (acc + acc[:, lane ^ d]).astype(np.float32)
        d *= 2
    return acc[:, 0]


def step32(X32, w32, mind, owner, c, fault=None, skip_from=None):
    """the kernel's update in fp32 (in place on copies): returns (mind, owner, radius)"""
    N = X32.shape[0]
    rows = np.arange(N)
    mind, owner = mind.copy(), owner.copy()
    d = (np.float32(1.0) - dot32(X32, X32[c])).astype(np.float32)
    radius = mind[c]
    with np.errstate(invalid="ignore"):
        take = (owner != rows) & ((d <= mind) if fault == "owner_le" else (d < mind))
    if fault == "overwrite":
        take = owner != rows
    take[c] = False
    if fault == "rows_skipped":
        take[skip_from:] = False
    mind[take], owner[take] = d[take], c
    mind[c], owner[c] = np.float32(0.0), c
    if fault == "radius_after":
        radius = mind[c]
    return mind, owner, radius


def scan32(w32, mind, owner, fault=None, skip_from=None):
    N = mind.shape[0]
    rows = np.arange(N)
    el = np.ones(N, dtype=bool) if fault == "centre_eligible" else owner != rows
    use_w = w32 is not None and fault != "weight_ignored"
    if w32 is not None and fault != "weight_ignored":
        with np.errstate(invalid="ignore"):
            el &= np.isnan(w32) | (w32 > 0) if fault == "nan_weight" else (w32 > 0)
    with np.errstate(invalid="ignore"):
        vals = (w32 * mind).astype(np.float32) if use_w else mind
    if fault == "rows_skipped":
        el[skip_from:] = False
    if fault == "nan_weight" and w32 is not None:
        vals = np.where(np.isnan(w32), np.float32(INF), vals)   # the defect: the NaN weight's key compares as the largest
    return argmax_key(vals, el, tie_high=fault == "tie_high")


def greedy32(X32, w32, m, seeds=(), first=None, fault=None, skip_from=None):
    """The whole selection as the kernel runs it (fp32, its order), optionally with one planted fault.  Seeds are placed
    by float64 distances rounded to fp32.  Returns dict(picks, radius, mind, owner)."""
    N = X32.shape[0]
    if len(seeds):
        st = seeded_state(X32.astype(np.float64), seeds)
        mind, owner = st["mind"].astype(np.float32), st["owner"]
    else:
        mind, owner = np.full(N, INF, dtype=np.float32), np.full(N, -1, dtype=np.int64)
    picks, radius = [], []
    nxt = scan32(w32, mind, owner, fault, skip_from)
    stale = nxt
    for t in range(m):
        if t == 0 and first is not None:
            c = int(first)
        else:
            c = stale if fault == "stale_partials" and t > 0 else nxt
        if c < 0:
            picks.append(-1); radius.append(np.float32("nan"))
            continue
        stale = nxt
        mind, owner, r = step32(X32, w32, mind, owner, c, fault, skip_from)
        picks.append(c); radius.append(r)
        nxt = scan32(w32, mind, owner, fault, skip_from)
    return dict(picks=np.array(picks, dtype=np.int64), radius=np.array(radius, dtype=np.float32), mind=mind, owner=owner)


# ---------------------------------------------------------------------------------------------------------------------------
# seeded test rows (torch only here: the rounding to the 16-bit type)


def unit_rows16(N, D, seed, dtype, scale=1.0):
    """N random directions, normalised in float64 and rounded once to `dtype`: a CPU torch tensor [N, D]"""
    import torch
    g = np.random.RandomState(seed)
    x = g.standard_normal((N, D))
    x = scale * x / np.linalg.norm(x, axis=1, keepdims=True)
    return torch.from_numpy(x).to(dtype)


def planted_clusters16(K, per, D, noise, seed, dtype):
    """K random directions with `per` rows around each (direction + noise * gaussian / sqrt(D), normalised), shuffled.  Returns
    (rows 16-bit CPU tensor [K per, D], cluster int64 numpy [K per])"""
    import torch
    g = np.random.RandomState(seed)
    dirs = g.standard_normal((K, D))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    cls = np.repeat(np.arange(K), per)
    x = dirs[cls] + noise / np.sqrt(D) * g.standard_normal((K * per, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    perm = g.permutation(K * per)
    return torch.from_numpy(x[perm]).to(dtype), cls[perm]


# the planted, well separated case of the end-to-end test: tests/test_coreset_cpu.py verifies on the host that the smallest gap
# between the best and the second-best key over its K picks is at least 100 x the tolerance of the two keys
PLANTED = dict(K=8, per=12, D=64, noise=0.25, seed=3)
