"""GPU: csrc/coreset.hip at the kernel boundary, through cclip_hip.ops, against the float64 reference and the derived bounds of
tests/coreset_ref.py.  Both 16-bit types; every team size (D = 32: 4 lanes, 64: 8, 96: a row that does not fill its 16 lanes,
512: a full wave, 544: a second pass that is partly empty, 1024: two full passes); N around the work-group's 64 rows and the
smallest N at which every work-group takes a second, partly empty, grid-stride trip; both row strides.  Keys are integers:
whatever the kernel selects from keys is compared exactly.  Every case prints `[coreset] name: largest err / tol`."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreset_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)
IDS = ["bf16", "fp16"]
DS = (32, 64, 96, 512, 544, 1024)
MASK = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ops():
    from cclip_hip import ops as o
    return o


def on_device(x16, pad=0):
    """the rows on the device with row stride D + pad"""
    N, D = x16.shape
    buf = torch.zeros(N, D + pad, dtype=x16.dtype, device="cuda")
    buf[:, :D] = x16.cuda()
    return buf[:, :D]


def fresh(N):
    return (torch.full((N,), float("inf"), device="cuda"), torch.full((N,), -1, dtype=torch.int32, device="cuda"))


def keys(ops, N):
    return torch.zeros(ops.coreset_blocks(N), dtype=torch.int64, device="cuda")


def score_key(v):
    v = np.float32(v) + np.float32(0.0)
    if np.isnan(v):
        return 0
    b = int(np.array(v, dtype=np.float32).view(np.uint32))
    return (~b & MASK) if b & 0x80000000 else (b | 0x80000000)


def best_key(w, mind, owner):
    """the largest key the kernel can form from the device's own fp32 state: exact"""
    N = len(mind)
    el = R.eligible(owner.astype(np.int64), w)
    with np.errstate(invalid="ignore"):
        vals = mind if w is None else (w * mind).astype(np.float32)
    return max([(score_key(vals[i]) << 32) | (~int(i) & MASK) for i in np.nonzero(el)[0]], default=0)


def top_key(k):
    return int(np.max(k.cpu().numpy().view(np.uint64))) if k.numel() else 0


def key_row(k):
    return -1 if k == 0 else (~k) & MASK


def second_trip_N(ops):
    """the smallest N at which every work-group takes a second grid-stride trip at D = 32 (64 rows a trip), the last one with a
    single row: all first trips, all but one full second trips, one row"""
    P = ops.coreset_blocks(2 ** 30)
    assert P == ops.coreset_blocks(P * 64) and ops.coreset_blocks((P - 1) * 64) == P - 1
    return P * 64 + (P - 1) * 64 + 1


def run_step(ops, x, w, mind, owner, kout, **kw):
    pick, radius = ops.coreset_step(x, mind, owner, kout, weight=w, **kw)
    torch.cuda.synchronize()
    return (None, None) if pick is None else (int(pick.item()), float(radius.item()))


def np_state(mind, owner):
    return mind.cpu().numpy().copy(), owner.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_given_centre_and_from_partials(ops, dtype, D, pad):
    N = 257
    x16 = R.unit_rows16(N, D, 100 + D, dtype)
    x, X = on_device(x16, pad), R.rows64(x16)
    g = np.random.RandomState(D)
    w_np = g.uniform(0.1, 2.0, N).astype(np.float32)
    worst = 0.0
    for w_host in (None, w_np):
        w = None if w_host is None else torch.from_numpy(w_host).cuda()
        w64 = None if w_host is None else w_host.astype(np.float64)
        mind, owner = fresh(N)                                          # the initial state: +inf / -1
        ka, kb = keys(ops, N), keys(ops, N)
        c0 = 200
        m0, o0 = np_state(mind, owner)
        pick, radius = run_step(ops, x, w, mind, owner, ka, centre=c0)
        m1, o1 = np_state(mind, owner)
        bad, ratio = R.check_step(X, w64, m0, o0, c0, m1, o1, radius)
        assert pick == c0 and radius == np.inf and not bad, bad
        worst = max(worst, ratio)
        assert top_key(ka) == best_key(w_host, m1, o1)
        # from the partials: exactly the row of the largest key; then a second given-centre state change on finite minima
        c1 = key_row(top_key(ka))
        pick, radius = run_step(ops, x, w, mind, owner, kb, partial_in=ka)
        m2, o2 = np_state(mind, owner)
        bad, ratio = R.check_step(X, w64, m1, o1, c1, m2, o2, radius)
        assert pick == c1 and not bad, bad
        worst = max(worst, ratio)
        assert top_key(kb) == best_key(w_host, m2, o2)
        # two launches from equal states are bitwise equal
        mind_b, owner_b = fresh(N)
        ka2, kb2 = keys(ops, N), keys(ops, N)
        run_step(ops, x, w, mind_b, owner_b, ka2, centre=c0)
        run_step(ops, x, w, mind_b, owner_b, kb2, partial_in=ka2)
        assert torch.equal(mind_b.view(torch.int32), mind.view(torch.int32)) and torch.equal(owner_b, owner)
        assert torch.equal(ka2, ka) and torch.equal(kb2, kb)
    print(f"[coreset] step D={D} ld={D + pad} {dtype}: largest err / tol = {worst:.4f}")


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, "second trip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sizes(ops, dtype, N):
    D = 32
    if N == "second trip":
        N = second_trip_N(ops)
    x16 = R.unit_rows16(N, D, N % 1000, dtype)
    x, X = on_device(x16), R.rows64(x16)
    mind, owner = fresh(N)
    ka, kb = keys(ops, N), keys(ops, N)
    c0 = N - 1
    m0, o0 = np_state(mind, owner)
    pick, radius = run_step(ops, x, None, mind, owner, ka, centre=c0)
    m1, o1 = np_state(mind, owner)
    bad, worst = R.check_step(X, None, m0, o0, c0, m1, o1, radius)
    assert pick == c0 and not bad, bad
    assert top_key(ka) == best_key(None, m1, o1)
    pick, radius = run_step(ops, x, None, mind, owner, kb, partial_in=ka)
    m2, o2 = np_state(mind, owner)
    if N == 1:
        assert pick == -1 and np.isnan(radius) and np.array_equal(m2, m1) and np.array_equal(o2, o1) and top_key(kb) == 0
    else:
        c1 = key_row(top_key(ka))
        bad, ratio = R.check_step(X, None, m1, o1, c1, m2, o2, radius)
        assert pick == c1 and not bad, bad
        worst = max(worst, ratio)
        assert top_key(kb) == best_key(None, m2, o2)
    print(f"[coreset] sizes N={N} D={D} {dtype}: largest err / tol = {worst:.4f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_garbage_partials_and_guard_bands(ops, dtype):
    N, D, G = 130, 96, 64
    x16 = R.unit_rows16(N, D, 9, dtype)
    x, X = on_device(x16), R.rows64(x16)
    P = ops.coreset_blocks(N)
    big_m = torch.full((N + 2 * G,), 123.0, device="cuda")
    big_o = torch.full((N + 2 * G,), 77, dtype=torch.int32, device="cuda")
    big_k = torch.full((P + 2 * G,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    big_p = torch.full((1 + 2 * G,), -99, dtype=torch.int32, device="cuda")
    big_r = torch.full((1 + 2 * G,), -5.0, device="cuda")
    mind, owner, kout = big_m[G:G + N], big_o[G:G + N], big_k[G:G + P]
    pick_t, rad_t = big_p[G:G + 1], big_r[G:G + 1]
    mind.fill_(float("inf")); owner.fill_(-1)
    ops.coreset_step(x, mind, owner, kout, centre=5, out_pick=pick_t, out_radius=rad_t)

    def bands_intact():
        torch.cuda.synchronize()
        for big, fill in ((big_m, 123.0), (big_o, 77), (big_k, 0x5A5A5A5A5A5A5A5A), (big_p, -99), (big_r, -5.0)):
            assert (big[:G] == fill).all() and (big[-G:] == fill).all()

    bands_intact()
    # keys whose rows lie far beyond N: the centre is clamped to the last row
    kin = np.array([(0xC0000000 << 32) | (~(N + 7 + 1000 * i) & MASK) for i in range(P)], dtype=np.uint64)
    kin = torch.from_numpy(kin.view(np.int64)).cuda()
    m0, o0 = np_state(mind, owner)
    ops.coreset_step(x, mind, owner, kout, partial_in=kin, out_pick=pick_t, out_radius=rad_t)
    bands_intact()
    m1, o1 = np_state(mind, owner)
    assert pick_t.item() == N - 1
    bad, ratio = R.check_step(X, None, m0, o0, N - 1, m1, o1, rad_t.item())
    assert not bad, bad
    # all keys zero: pick -1, radius NaN, nothing updated; the scan still reports the state
    ops.coreset_step(x, mind, owner, kout, partial_in=torch.zeros(P, dtype=torch.int64, device="cuda"), out_pick=pick_t, out_radius=rad_t)
    bands_intact()
    m2, o2 = np_state(mind, owner)
    assert pick_t.item() == -1 and np.isnan(rad_t.item()) and np.array_equal(m2, m1) and np.array_equal(o2, o1)
    assert top_key(kout) == best_key(None, m2, o2)
    # scan only: the same keys, no update, pick / radius untouched
    kout2 = keys(ops, N)
    assert ops.coreset_step(x, mind, owner, kout2, scan_only=True) == (None, None)
    torch.cuda.synchronize()
    assert torch.equal(kout2, kout) and pick_t.item() == -1
    print(f"[coreset] garbage partials {dtype}: largest err / tol = {ratio:.4f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_duplicates_centres_and_weights(ops, dtype):
    N, D = 200, 64
    x16 = R.unit_rows16(N, D, 31, dtype)
    x16[150] = x16[20]; x16[90] = x16[20]                  # equal rows carry equal keys: the lower row wins
    x, X = on_device(x16), R.rows64(x16)
    g = np.random.RandomState(4)
    w_rand = g.uniform(0.05, 3.0, N).astype(np.float32)
    w_holes = w_rand.copy(); w_holes[::3] = 0.0; w_holes[[20, 90, 7]] = np.nan; w_holes[150] = 2.0
    worst = 0.0
    for name, w_host, m in (("none", None, N), ("random", w_rand, 60), ("zero and NaN", w_holes, 140), ("all zero", np.zeros(N, dtype=np.float32), 3)):
        w = None if w_host is None else torch.from_numpy(w_host).cuda()
        mind, owner = fresh(N)
        first = 0 if w_host is None else int(np.nonzero(np.nan_to_num(w_host) > 0)[0][0]) if (np.nan_to_num(w_host) > 0).any() else 0
        picks, radius, _ = ops.coreset_greedy(x, mind, owner, m, first=first, weight=w)
        torch.cuda.synchronize()
        p, r = picks.cpu().numpy().astype(np.int64), radius.cpu().numpy()
        live = p[p >= 0]
        assert len(set(live.tolist())) == len(live), "a centre was selected again"
        if name == "all zero":
            assert p.tolist() == [0, -1, -1] and np.isnan(r[1:]).all()
            continue
        w64 = None if w_host is None else w_host.astype(np.float64)
        md, ow = np_state(mind, owner)
        bad, ratio = R.check_selection(X, w64, p, r, md.astype(np.float64), ow, first=first)
        assert not bad, bad
        worst = max(worst, ratio)
        if name == "none":
            assert sorted(p.tolist()) == list(range(N)) and (md == 0).all() and (ow == np.arange(N)).all()
            where = {int(v): t for t, v in enumerate(p)}
            assert where[20] < where[90] < where[150]
        if name == "zero and NaN":
            elig = np.nan_to_num(w_host) > 0
            assert elig[live[1:]].all() and (p >= 0).sum() == min(m, 1 + elig.sum() - elig[first])
    print(f"[coreset] duplicates / weights {dtype}: largest err / tol = {worst:.4f}")


@pytest.mark.parametrize("D", [32, 544])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_row_does_not_feel_its_position_or_N(ops, dtype, D):
    base = R.unit_rows16(300, D, 77, dtype)
    probe, centre = base[5], base[6]
    bits = []
    for N, at, c in ((66, 1, 0), (66, 65, 33), (300, 257, 299), (second_trip_N(ops) if D == 32 else 1500, 1203, 64)):
        x16 = R.unit_rows16(N, D, N, dtype)
        x16[at], x16[c] = probe, centre
        x = on_device(x16)
        mind, owner = fresh(N)
        mind[at] = 3.0                                          # an old minimum every cosine distance beats
        ops.coreset_step(x, mind, owner, keys(ops, N), centre=c)
        bits.append((mind[at:at + 1].view(torch.int32).item(), owner[at].item() == c))
    assert len(set(bits)) == 1 and bits[0][1], bits


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_greedy_equals_single_steps_bit_for_bit(ops, dtype, weighted):
    N, D, m = 1000, 96, 37
    x = on_device(R.unit_rows16(N, D, 12, dtype), 8)
    w = torch.rand(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) if weighted else None
    mind_a, owner_a = fresh(N)
    picks, radius, ws = ops.coreset_greedy(x, mind_a, owner_a, m, first=17, weight=w)
    mind_b, owner_b = fresh(N)
    kk = [keys(ops, N), keys(ops, N)]
    got_p, got_r = [], []
    for t in range(m):
        p, r = ops.coreset_step(x, mind_b, owner_b, kk[(t + 1) % 2], weight=w, **(dict(centre=17) if t == 0 else dict(partial_in=kk[t % 2])))
        got_p.append(p); got_r.append(r)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(got_p), picks) and torch.equal(torch.cat(got_r).view(torch.int32), radius.view(torch.int32))
    assert torch.equal(mind_a.view(torch.int32), mind_b.view(torch.int32)) and torch.equal(owner_a, owner_b)
    assert torch.equal(ws[m % 2], kk[m % 2])
    # a second call continues from the keys the first left: the same as one call of both lengths
    mind_c, owner_c = fresh(N)
    p1, r1, ws_c = ops.coreset_greedy(x, mind_c, owner_c, 10, first=17, weight=w)
    if 10 % 2:
        ws_c = ws_c.flip(0).contiguous()
    p2, r2, _ = ops.coreset_greedy(x, mind_c, owner_c, m - 10, workspace=ws_c, weight=w)
    assert torch.equal(torch.cat([p1, p2]), picks) and torch.equal(mind_c.view(torch.int32), mind_a.view(torch.int32))
    assert ops.coreset_greedy(x, mind_c, owner_c, 0, workspace=ws_c)[0].numel() == 0


def test_every_argument_error_leaves_the_outputs_alone(ops):
    from cclip_hip._lib import lib
    N, D = 70, 64
    x = on_device(R.unit_rows16(N, D, 1, torch.bfloat16), 8)
    P = ops.coreset_blocks(N)
    assert P == 2 and ops.coreset_workspace(N) == 2 * P * 8 and ops.coreset_blocks(0) == 0 and ops.coreset_workspace(2 ** 31) == 0
    mind, owner = fresh(N)
    ws = torch.full((2, P), 5, dtype=torch.int64, device="cuda")
    pick = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    rad = torch.full((4,), -7.0, device="cuda")
    wt = torch.ones(N + 1, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

    def step(**kw):
        a = dict(x=x.data_ptr(), ldx=x.stride(0), N=N, D=D, weight=0, mind=mind.data_ptr(), owner=owner.data_ptr(), centre=-1,
                 pin=ws[0].data_ptr(), pout=ws[1].data_ptr(), pick=pick.data_ptr(), rad=rad.data_ptr())
        a.update(kw)
        return lib.cclip_coreset_step(vp(a["x"]), i64(a["ldx"]), i64(a["N"]), i32(a["D"]), vp(a["weight"]), vp(a["mind"]), vp(a["owner"]),
                                      i32(a["centre"]), vp(a["pin"]), vp(a["pout"]), vp(a["pick"]), vp(a["rad"]), stream)

    def greedy(**kw):
        a = dict(x=x.data_ptr(), ldx=x.stride(0), N=N, D=D, weight=0, mind=mind.data_ptr(), owner=owner.data_ptr(), first=0, m=3,
                 picks=pick.data_ptr(), rad=rad.data_ptr(), ws=ws.data_ptr(), nbytes=2 * P * 8)
        a.update(kw)
        return lib.cclip_coreset_greedy(vp(a["x"]), i64(a["ldx"]), i64(a["N"]), i32(a["D"]), vp(a["weight"]), vp(a["mind"]), vp(a["owner"]),
                                        i32(a["first"]), i64(a["m"]), vp(a["picks"]), vp(a["rad"]), vp(a["ws"]), i64(a["nbytes"]), stream)

    shared = [dict(x=0), dict(mind=0), dict(owner=0), dict(x=x.data_ptr() + 2), dict(N=0), dict(N=-3), dict(N=2 ** 31), dict(D=0),
              dict(D=16), dict(D=48), dict(D=1056), dict(ldx=D - 8), dict(ldx=D + 4), dict(weight=wt.data_ptr() + 2),
              dict(mind=mind.data_ptr() + 2), dict(owner=owner.data_ptr() + 2), dict(pick=pick.data_ptr() + 2), dict(rad=rad.data_ptr() + 2)]
    for bad in shared + [dict(pout=0), dict(pin=0), dict(pin=ws[1].data_ptr()), dict(pout=ws[1].data_ptr() + 4), dict(pin=ws[0].data_ptr() + 4),
                         dict(centre=-3), dict(centre=N), dict(pick=0), dict(rad=0), dict(centre=3, pick=0)]:
        assert step(**bad) == 1, bad
    for bad in shared[:-2] + [dict(picks=pick.data_ptr() + 2), dict(rad=rad.data_ptr() + 2), dict(m=-1), dict(m=N + 1), dict(first=-2), dict(first=N),
                              dict(ws=0), dict(ws=ws.data_ptr() + 4), dict(nbytes=2 * P * 8 - 1), dict(picks=0), dict(rad=0)]:
        assert greedy(**bad) == 1, bad
    torch.cuda.synchronize()
    assert torch.isinf(mind).all() and (owner == -1).all() and (ws == 5).all() and (pick == -7).all() and (rad == -7.0).all()
    assert greedy(m=0, picks=0, rad=0) == 0 and step(centre=-2, pick=0, rad=0, pin=0) == 0          # the legal nulls
    torch.cuda.synchronize()
    assert torch.isinf(mind).all() and (pick == -7).all()
    for bad in (dict(centre=N), dict(centre=-1)):
        with pytest.raises(ValueError):
            ops.coreset_step(x, mind, owner, ws[1], **bad)
    with pytest.raises(ValueError):
        ops.coreset_step(x, mind, owner, ws[1], partial_in=ws[1])
    with pytest.raises(TypeError):
        ops.coreset_step(x.cpu(), mind, owner, ws[1], centre=0)
    with pytest.raises(NotImplementedError):
        ops.coreset_step(torch.zeros(4, 48, dtype=torch.bfloat16, device="cuda"), mind[:4].clone(), owner[:4].clone(), ws[1], centre=0)
