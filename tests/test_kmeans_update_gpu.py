"""The centroid step of k-means on the MI355X (cclip_kmeans_update, csrc/embed_kmeans.hip) against float64 on the same 16-bit
rows (tests/kmeans_ref.py): sums, norms and unit rows within the derived three-part bound written out there, empty and
cancelling clusters, exact counts, bitwise repeatability, argument errors.

How a unit row is compared (rule of the band).  With c the float64 value and f32_tol the fp32 part of the bound, the kernel's
16-bit output must lie between round16(c - f32_tol) and round16(c + f32_tol) - where the two agree that is equality with the
once-rounded float64 value - and it may never be more than ONE 16-bit step from round16(c), however wide the bound is.  The
share of elements whose two ends differ is a property of the inputs: it is computed on the reference alone and asserted
before the kernel runs, over the clusters of at most 256 rows (one slab; above, n 2^-24 sum|x| grows past the 16-bit spacing
and the band covers everything, which is why the one-step rule stands on its own): at most BAND_CAP of their elements.
For such a cluster the bound is <= 256 * 2^-24 * rho relative with rho = sum|x| / |sum x| ~ 1 for the planted rows, against a
half spacing of >= 2^-12 relative in fp16: a share of about 2 * 1.5e-5 / 2.4e-4 = 12 % at 256 rows, far less on average.

Every case prints its figures (`[kmeans-update] ...`) before it asserts; run with -s to collect them.
"""
import functools

import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
BAND_CAP = 0.15
SLAB = 256

# (N, K, D) -> the first cluster sizes; the rest of the rows is dealt at random over the remaining clusters (some stay empty).
# Between them: an empty cluster, a cluster of one row, one cluster with 90 % of the rows (crosses many slabs), clusters that
# start or end exactly on a slab boundary (the running sums 256, 768, 45056 = 176 * 256)
CASES = {
    (1, 1, 32): [1],
    (5, 3, 128): [1, 0, 4],
    (300, 7, 768): [1, 0, 255, 20, 0, 14, 10],
    (4097, 64, 512): [256, 512, 1, 0],
    (20000, 3, 96): [18000, 1, 1999],
    (50000, 1000, 160): [45000, 0, 1, 55],
}


@functools.lru_cache(maxsize=None)
def case_inputs(N, K, D, dtype):
    """rows around one direction per cluster, dealt to the rows by a random permutation; the reference, computed once"""
    gen = torch.Generator().manual_seed(100 * D + N + K)
    head = CASES[(N, K, D)]
    sizes = torch.zeros(K, dtype=torch.int64)
    sizes[:len(head)] = torch.tensor(head)
    rest = N - int(sizes.sum())
    if rest:
        sizes[len(head):] += torch.bincount(torch.randint(len(head), K, (rest,), generator=gen), minlength=K)[len(head):]
    assert int(sizes.sum()) == N
    assign = torch.empty(N, dtype=torch.int64)
    assign[torch.randperm(N, generator=gen)] = torch.repeat_interleave(torch.arange(K), sizes)
    dirs = torch.randn(K, D, generator=gen)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    x = dirs[assign] + 0.3 / D ** 0.5 * torch.randn(N, D, generator=gen)
    x16 = (x / x.norm(dim=1, keepdim=True)).to(dtype)
    prev16 = torch.randn(K, D, generator=gen).to(dtype)
    return x16, assign, prev16, R.update_ref(x16, assign, K, prev16)


def ordinal(t16):
    """the 16-bit patterns as integers in value order"""
    b = t16.view(torch.int16).int() & 0xffff
    return torch.where(b < 0x8000, b, 0x8000 - b)


def band_condition(r, dtype, what):
    """on the reference alone: the two ends of every element and the share of the band among the clusters of one slab"""
    live = ~r["keep"]
    lo16, hi16 = R.round16(r["c"] - r["f32_tol"], dtype), R.round16(r["c"] + r["f32_tol"], dtype)
    band = (ordinal(lo16) != ordinal(hi16)) & live[:, None]
    small = live & (r["counts"] <= SLAB)
    share = band[small].float().mean().item() if small.any() else 0.0
    print(f"[kmeans-update] {what}: clusters {int(live.sum())} live / {int(small.sum())} of one slab, band share there {share:.4f}, "
          f"overall {band[live].float().mean().item() if live.any() else 0.0:.4f}, max eta {r['eta'][live].max().item() if live.any() else 0:.3e}")
    assert share <= BAND_CAP, f"{what}: {share:.3f} of the elements lie within the fp32 bound of a rounding boundary"
    assert (r["eta"][live] < 0.5).all()
    return lo16, hi16, band


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,K,D", list(CASES))
def test_kernel_against_float64(N, K, D, dtype):
    from cclip_hip import ops
    x16, assign, prev16, r = case_inputs(N, K, D, dtype)
    what = f"N{N} K{K} D{D} {dtype}"
    lo16, hi16, band = band_condition(r, dtype, what)
    xd, ad, pd = x16.cuda(), assign.cuda(), prev16.cuda()
    c1, n1, k1 = ops.kmeans_update(xd, ad, K, pd)
    c2, n2, k2 = ops.kmeans_update(xd, ad.int(), K, pd)
    torch.cuda.synchronize()
    assert c1.dtype == dtype and c1.shape == (K, D) and n1.dtype == torch.float32 and n1.shape == (K,) and k1.dtype == torch.int64
    assert torch.equal(c1.view(torch.int16), c2.view(torch.int16)) and torch.equal(n1.view(torch.int32), n2.view(torch.int32)) and \
        torch.equal(k1, k2), "two launches differ"
    c, nrm, cnt = c1.cpu(), n1.cpu().double(), k1.cpu()
    assert torch.equal(cnt, r["counts"]), "counts"
    keep, live = r["keep"], ~r["keep"]
    assert torch.equal(c[keep].view(torch.int16), prev16[keep].view(torch.int16)), "an empty cluster must keep prev_c bit for bit"
    assert (nrm[keep] == 0).all()
    nerr = ((nrm - r["norm"]).abs() / r["norm_tol"])[live].max().item()
    oc, olo, ohi, oref = ordinal(c), ordinal(lo16), ordinal(hi16), ordinal(R.round16(r["c"], dtype))
    outside = ((oc < olo) | (oc > ohi))[live]
    steps = (oc - oref).abs()[live]
    cerr = ((c.double() - r["c"]).abs())[live].max().item()
    print(f"[kmeans-update] {what}: norm err / tol {nerr:.3e}; unit rows: max |err| {cerr:.3e}, outside the ends {int(outside.sum())}, "
          f"one step off {int((steps == 1).sum())} (in the band {int(((oc != oref) & band)[live].sum())}), further {int((steps > 1).sum())}")
    assert nerr <= 1.0, f"{what}: a norm is {nerr:.3f} of its bound off"
    assert not outside.any(), f"{what}: {int(outside.sum())} elements outside round16(c -/+ f32_tol)"
    assert (steps <= 1).all(), f"{what}: an element is more than one 16-bit step from the rounded float64 value"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rows_that_cancel_keep_the_previous_centroid(dtype):
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(8)
    N, K, D = 601, 4, 64
    x16 = torch.randint(-8, 9, (N, D), generator=gen).to(dtype)                 # small integers: every fp32 sum below is exact
    x16[300:600] = -x16[:300]                                                   # a row and its mirror
    half = torch.randint(0, 2, (300,), generator=gen)
    assign = torch.cat([half, half, torch.tensor([3])])                         # clusters 0 and 1 cancel to zero, 2 is empty
    assign[[5, 305]] = 3                                                        # cluster 3: a pair that cancels and one more row
    prev = torch.randn(K, D, generator=gen).to(dtype)
    c, nrm, cnt = ops.kmeans_update(x16.cuda(), assign.cuda(), K, prev.cuda())
    c, nrm, cnt = c.cpu(), nrm.cpu(), cnt.cpu()
    assert torch.equal(cnt, torch.bincount(assign, minlength=K)) and cnt[2] == 0 and cnt[3] == 3
    assert torch.equal(c[:3].view(torch.int16), prev[:3].view(torch.int16)) and nrm[:3].tolist() == [0.0, 0.0, 0.0]
    r = R.update_ref(x16, assign, K, prev)
    assert abs(nrm[3].item() - r["norm"][3].item()) <= r["norm_tol"][3].item()
    o = ordinal(c[3])
    assert ((o >= ordinal(R.round16(r["c"][3] - r["f32_tol"][3], dtype))) & (o <= ordinal(R.round16(r["c"][3] + r["f32_tol"][3], dtype)))).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_outputs_in_place_and_strided(dtype):
    from cclip_hip import ops
    x16, assign, prev16, r = case_inputs(300, 7, 768, dtype)
    xd, ad = x16.cuda(), assign.cuda()
    want_c, want_n, _ = ops.kmeans_update(xd, ad, 7, prev16.cuda())
    wide = torch.zeros(300, 768 + 64, device="cuda", dtype=dtype)
    wide[:, 32:800] = xd
    buf = torch.zeros(7, 1024, device="cuda", dtype=dtype)
    buf[:, :768] = prev16.cuda()
    norm = torch.empty(7, device="cuda")
    c, n, _ = ops.kmeans_update(wide[:, 32:800], ad, 7, buf[:, :768], out_c=buf[:, :768], out_norm=norm)   # out_c is prev_c itself
    assert n is norm and c.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, :768].contiguous().view(torch.int16), want_c.view(torch.int16)) and torch.equal(n.view(torch.int32), want_n.view(torch.int32))
    assert not buf[:, 768:].any(), "the columns beyond D were written"


def test_argument_errors():
    from cclip_hip import ops
    x = torch.randn(100, 64, device="cuda").bfloat16()
    prev = torch.randn(4, 64, device="cuda").bfloat16()
    a = torch.randint(0, 4, (100,), device="cuda")
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        ops.kmeans_update(x, torch.where(a == 0, 4, a), 4, prev)
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        ops.kmeans_update(x, a - 1, 4, prev)
    with pytest.raises(ValueError, match="prev_c has 4 rows"):
        ops.kmeans_update(x, a, 5, prev)
    with pytest.raises(ValueError, match="assign"):
        ops.kmeans_update(x, a[:99], 4, prev)
    with pytest.raises(TypeError, match="int32 or int64"):
        ops.kmeans_update(x, a.float(), 4, prev)
    with pytest.raises(TypeError, match="cuda"):
        ops.kmeans_update(x, a.cpu(), 4, prev)
    with pytest.raises(TypeError, match="cuda"):
        ops.kmeans_update(x.cpu(), a, 4, prev)
    with pytest.raises(TypeError, match="mixed"):
        ops.kmeans_update(x, a, 4, prev.half())
    with pytest.raises(ValueError, match="columns"):
        ops.kmeans_update(x, a, 4, torch.randn(4, 96, device="cuda").bfloat16())
    with pytest.raises(ValueError, match="empty"):
        ops.kmeans_update(x[:0], a[:0], 4, prev)
    with pytest.raises(NotImplementedError, match="D % 32 == 0"):
        ops.kmeans_update(torch.randn(100, 40, device="cuda").bfloat16(), a, 4, torch.randn(4, 40, device="cuda").bfloat16())
    with pytest.raises(ValueError, match="out_c"):
        ops.kmeans_update(x, a, 4, prev, out_c=torch.empty(4, 64, device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError, match="out_norm"):
        ops.kmeans_update(x, a, 4, prev, out_norm=torch.empty(5, device="cuda"))
    torch.cuda.synchronize()


def test_c_entry_refuses_bad_arguments():
    """the same limits at the C ABI: CCLIP_ERR_ARG (1), nothing launched"""
    import ctypes
    from cclip_hip import load_library, ops
    lib = load_library()
    P, L, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    N, K, D = 600, 4, 64
    assert ops.kmeans_update_workspace(N, K, D) == (3 + 4) * 64 * 4
    assert ops.kmeans_update_workspace(0, K, D) == 0 and ops.kmeans_update_workspace(N, 0, D) == 0 and ops.kmeans_update_workspace(N, K, 40) == 0
    assert ops.kmeans_update_workspace(2 ** 31, K, D) == 0 and ops.kmeans_update_workspace(N, K, 1056) == 0
    x = torch.randn(N, 72, device="cuda").bfloat16()
    order = torch.arange(N, device="cuda", dtype=torch.int32)
    seg = torch.tensor([0, 100, 100, 350, 600], device="cuda", dtype=torch.int32)
    prev = torch.randn(K, D, device="cuda").bfloat16()
    out = torch.empty(K, D, device="cuda", dtype=torch.bfloat16)
    norm = torch.empty(K + 1, device="cuda")
    nbytes = ops.kmeans_update_workspace(N, K, D)
    ws = torch.empty(nbytes // 4 + 1, device="cuda")

    def call(xp=x.data_ptr(), ldx=72, N_=N, D_=D, op=order.data_ptr(), sp=seg.data_ptr(), K_=K, pp=prev.data_ptr(), ldp=D, cp=out.data_ptr(),
             ldo=D, np_=norm.data_ptr(), wp=ws.data_ptr(), wb=nbytes, fn=lib.cclip_kmeans_update):
        return fn(P(xp), L(ldx), L(N_), I(D_), P(op), P(sp), L(K_), P(pp), L(ldp), P(cp), L(ldo), P(np_), P(wp), L(wb), P(0))

    assert call() == 0 and call(fn=lib.cclip_kmeans_update_f16) == 0
    for bad in (dict(D_=40), dict(D_=0), dict(D_=1056), dict(N_=0), dict(N_=2 ** 31), dict(K_=0), dict(K_=2 ** 31), dict(ldx=68), dict(ldx=56),
                dict(xp=x.data_ptr() + 8), dict(xp=0), dict(op=0), dict(sp=0), dict(pp=0), dict(cp=0), dict(np_=0), dict(wp=0),
                dict(ldp=32), dict(ldo=63), dict(op=order.data_ptr() + 2), dict(sp=seg.data_ptr() + 2), dict(np_=norm.data_ptr() + 2),
                dict(wp=ws.data_ptr() + 2), dict(pp=prev.data_ptr() + 1), dict(cp=out.data_ptr() + 1), dict(wb=nbytes - 4)):
        assert call(**bad) == 1, bad
    torch.cuda.synchronize()
