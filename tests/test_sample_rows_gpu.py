"""cclip_sample_rows (csrc/sample_rows.hip) against the float64 restatement of its contract (tests/sample_ref.py).

Acceptance, per row and with no row excluded, at eps = 1e-4 (the bound fp32 kernels are held to against float64 here:
KERNEL_TOL of tests/test_relevance_gpu.py; masses are fractions of 1):
  * n_kept between the float64 kept-set sizes at top_p - eps and top_p + eps (so exactly min(k, V) where top-k alone binds);
  * with K = the first n_kept tokens of the exact order: |kept_mass - Z64| <= eps, the token lies in K, u * Z64 lies in
    [C_excl(token) - eps, C_incl(token) + eps] (C = the float64 running mass over K in id order), and
    |logprob - log p64[token]| <= 1e-4.
test_acceptance prints the largest deviations of its cases (`pytest -m gpu tests/test_sample_rows_gpu.py -s`).

The exact cases at u = 0 and u = 1 - 2^-24 ask for the lowest / highest kept id with nonzero p.  The draw rule compares a
running mass with u * Z, so the highest id is only reached when its own p exceeds 2^-24 Z, in float64 as much as on the
device; those two cases therefore run on rows whose finite logits lie in [-1, 1] (every finite token's p is above 1e-4 / V of
the row, far from both 0 and 2^-24), a third of the entries -inf (p exactly 0: never drawn)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sample_ref import FREQ_ROWS, draw_ref, frequency_bound_ok, frequency_case, sample_rows_ref  # noqa: E402

EPS = 1e-4
SIZES = [1, 2, 63, 64, 65, 257, 1000, 21128, 50257]
VARIANTS = ("normal", "ties", "spike", "neginf")
U_LAST = 1.0 - 2.0 ** -24


def _logits(variant, n, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, V, generator=g) * 3
    if variant == "ties":
        x = (x * 2).round() / 2                                          # multiples of 0.5: many exact ties
    elif variant == "spike":
        x[torch.arange(n), torch.randint(0, V, (n,), generator=g)] = 100.0
    elif variant == "neginf":
        drop = torch.rand(n, V, generator=g) < 1 / 3
        drop[torch.arange(n), torch.randint(0, V, (n,), generator=g)] = False      # (a finite logit in every row)
        x[drop] = float("-inf")
    return x


def _launch(x, u, *, inv_t=1.0, top_k=0, top_p=1.0, stop=-1, done=None, ld=None):
    from cclip_hip import ops
    n, V = x.shape
    if ld is None:
        xd = x.cuda()
    else:
        buf = torch.full((n, ld), float("nan"))                          # what lies between the rows must never be read
        buf[:, :V] = x
        xd = buf.cuda()[:, :V]
    done = torch.zeros(n, dtype=torch.int32) if done is None else done
    dd = done.cuda()
    tok, lp, nk, km = ops.sample_rows(xd, torch.as_tensor(u, dtype=torch.float32).cuda(), dd, inv_temperature=inv_t, top_k=top_k,
                                      top_p=top_p, stop_token=stop)
    return tok.cpu().numpy(), lp.cpu().numpy(), nk.cpu().numpy(), km.cpu().numpy(), dd.cpu().numpy()


class _Worst:
    def __init__(self):
        self.v = dict(kept_mass=0.0, cut=0.0, logprob=0.0, n_kept_off_exact=0)

    def up(self, k, x):
        self.v[k] = max(self.v[k], float(x))


def _check_rows(refs, u, out, top_p, worst):
    tok, lp, nk, km, _ = out
    for r, ref in enumerate(refs):
        ref.top_p = top_p
        lo, hi = ref.n_kept(top_p - EPS), ref.n_kept(top_p + EPS)
        assert lo <= nk[r] <= hi, (r, lo, int(nk[r]), hi)
        worst.up("n_kept_off_exact", abs(int(nk[r]) - ref.n_kept()))
        ids = ref.kept(int(nk[r]))
        c = np.cumsum(ref.p[ids])
        Z = c[-1]
        assert abs(km[r] - Z) <= EPS, (r, km[r], Z)
        worst.up("kept_mass", abs(km[r] - Z))
        at = int(np.searchsorted(ids, tok[r]))
        assert at < len(ids) and ids[at] == tok[r], (r, int(tok[r]), "not in the kept set")
        c_excl, c_incl, target = (c[at - 1] if at else 0.0), c[at], float(u[r]) * Z
        assert c_excl - EPS <= target <= c_incl + EPS, (r, int(tok[r]), c_excl, target, c_incl)
        worst.up("cut", max(c_excl - target, target - c_incl, 0.0))
        want = np.log(ref.p[tok[r]])
        assert abs(lp[r] - want) <= 1e-4, (r, int(tok[r]), lp[r], want)
        worst.up("logprob", abs(lp[r] - want))


@pytest.mark.parametrize("V", SIZES)
def test_acceptance(V):
    """every input variant x temperature x top_k x top_p at this V, three rows each; V = 257 also with 1 and 130 rows"""
    worst = _Worst()
    g = torch.Generator().manual_seed(1000 + V)
    for n in ((1, 3, 130) if V == 257 else (3,)):
        for vi, variant in enumerate(VARIANTS):
            x = _logits(variant, n, V, 7 * V + vi)
            for temperature in (0.5, 1.0, 2.0):
                inv_t = 1.0 / temperature
                refs = sample_rows_ref(x.numpy(), inv_t, 0, 1.0)
                for top_k in (0, 1, 5, V, V + 10):
                    for ref in refs:
                        ref.k = V if top_k <= 0 or top_k >= V else top_k
                    for top_p in ((1.0, 0.8, 1e-6) if n == 3 else (0.8,)):
                        u = torch.rand(n, generator=g).numpy()
                        _check_rows(refs, u, _launch(x, u, inv_t=inv_t, top_k=top_k, top_p=top_p), top_p, worst)
    print(f"V={V}: largest deviations {worst.v}")


@pytest.mark.parametrize("V,n", [(1000, 3), (21128, 130)])
def test_padded_rows_and_many_rows(V, n):
    worst = _Worst()
    x = _logits("ties", n, V, 5)
    u = torch.rand(n, generator=torch.Generator().manual_seed(6)).numpy()
    refs = sample_rows_ref(x.numpy(), 1.0, 0, 0.8)
    _check_rows(refs, u, _launch(x, u, top_p=0.8, ld=V + 5), 0.8, worst)
    print(f"V={V} n={n} ld=V+5: largest deviations {worst.v}")


@pytest.mark.parametrize("top_k", [0, 5])
def test_first_and_last_kept_token(top_k):
    V, n = 1000, 4
    g = torch.Generator().manual_seed(21)
    x = torch.rand(n, V, generator=g) * 2 - 1
    x[torch.rand(n, V, generator=g) < 1 / 3] = float("-inf")
    refs = sample_rows_ref(x.numpy(), 1.0, top_k, 1.0)
    for u, pick in ((0.0, 0), (U_LAST, -1)):
        tok, _, nk, _, _ = _launch(x, np.full(n, u, dtype=np.float32), top_k=top_k)
        for r, ref in enumerate(refs):
            ids = ref.kept()
            live = ids[ref.p[ids] > 0]
            assert nk[r] == (V if top_k == 0 else top_k) and len(live) >= 2
            assert tok[r] == live[pick] == draw_ref(ref, u)[0], (r, u, int(tok[r]), int(live[pick]))


@pytest.mark.parametrize("V", [2, 64, 65, 1000, 21128])
def test_one_token_filters_give_the_argmax_for_any_u(V):
    n = 6
    x = _logits("ties", n, V, 31)
    want = x.argmax(dim=1).numpy()                                       # the first maximum: ties go to the lowest id
    p = sample_rows_ref(x.numpy(), 1.0, 0, 1.0)
    for kw in (dict(top_k=1), dict(top_p=1e-6)):
        for u in (0.0, 0.37, U_LAST):
            tok, lp, nk, km, _ = _launch(x, np.full(n, u, dtype=np.float32), **kw)
            assert np.array_equal(tok, want) and (nk == 1).all()
            assert all(abs(lp[r] - np.log(p[r].p[want[r]])) <= 1e-4 and abs(km[r] - p[r].p[want[r]]) <= EPS for r in range(n))


def test_done_rows_and_the_stop_token():
    V, n = 63, 130
    x = _logits("normal", n, V, 41)
    u = torch.rand(n, generator=torch.Generator().manual_seed(42)).numpy()
    free = _launch(x, u)[0]
    stop = int(np.bincount(free[np.arange(n) % 3 != 0], minlength=V).argmax())                  # a token several rows draw
    entered = (torch.arange(n) % 3 == 0).to(torch.int32) * 5             # any nonzero value means done, and is left as it is
    tok, lp, nk, km, done = _launch(x, u, stop=stop, done=entered.clone())
    was = entered.numpy() != 0
    assert (tok[was] == 0).all() and (lp[was] == 0).all() and np.array_equal(done[was], entered.numpy()[was])
    assert np.array_equal(tok[~was], free[~was])
    assert np.array_equal(done[~was], (tok[~was] == stop).astype(np.int32))
    assert (tok[~was] == stop).sum() >= 2 and (tok[~was] != stop).sum() >= 2


def test_two_launches_are_bitwise_equal():
    x = _logits("ties", 64, 21128, 51)
    u = torch.rand(64, generator=torch.Generator().manual_seed(52)).numpy()
    a = _launch(x, u, inv_t=2.0, top_p=0.8, top_k=200)
    b = _launch(x, u, inv_t=2.0, top_p=0.8, top_k=200)
    for p, q in zip(a, b):
        assert p.tobytes() == q.tobytes()
    alone = _launch(x[5:6], u[5:6], inv_t=2.0, top_p=0.8, top_k=200)     # a row's outputs do not depend on the rows around it
    assert all(p[5:6].tobytes() == q.tobytes() for p, q in zip(a, alone))


def test_frequencies():
    logits, u, p = frequency_case()
    x = torch.from_numpy(logits).repeat(FREQ_ROWS, 1)
    tok, _, nk, km, _ = _launch(x, u)
    assert (nk == 64).all() and np.abs(km - 1).max() <= EPS
    ok, worst = frequency_bound_ok(np.bincount(tok, minlength=64), p)
    print(f"largest deviation {worst:.2f} binomial standard deviations")
    assert ok, worst


def test_bad_arguments_return_err_arg():
    from cclip_hip._lib import check, lib
    c_int, c_long, c_float, c_void_p = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    n, V = 2, 40
    t = dict(logits=torch.zeros(n, V, device="cuda"), u=torch.zeros(n, device="cuda"), done=torch.zeros(n, dtype=torch.int32, device="cuda"),
             token=torch.full((n,), -7, dtype=torch.int32, device="cuda"), logprob=torch.zeros(n, device="cuda"),
             n_kept=torch.zeros(n, dtype=torch.int32, device="cuda"), kept_mass=torch.zeros(n, device="cuda"))

    def call(null=None, **kw):
        a = dict(ld=V, n=n, V=V, inv_t=1.0, top_k=0, top_p=1.0)
        a.update(kw)
        p = {k: c_void_p(0 if k == null else v.data_ptr()) for k, v in t.items()}
        check(lib.cclip_sample_rows(p["logits"], c_long(a["ld"]), c_int(a["n"]), c_int(a["V"]), c_float(a["inv_t"]), c_int(a["top_k"]),
                                    c_float(a["top_p"]), p["u"], c_int(-1), p["done"], p["token"], p["logprob"], p["n_kept"],
                                    p["kept_mass"], c_void_p(torch.cuda.current_stream().cuda_stream)), "cclip_sample_rows")

    for kw in ([dict(null=k) for k in t] +
               [dict(n=0), dict(n=-1), dict(V=0), dict(V=65537, ld=65537), dict(ld=V - 1), dict(top_k=-1), dict(top_p=0.0),
                dict(top_p=1.5), dict(top_p=float("nan")), dict(inv_t=0.0), dict(inv_t=-1.0), dict(inv_t=float("nan"))]):
        with pytest.raises(RuntimeError, match="status 1"):
            call(**kw)
    torch.cuda.synchronize()
    assert (t["token"] == -7).all()                                      # nothing was launched
    call()
    torch.cuda.synchronize()
    assert (t["token"] == 0).all()                                       # all-equal logits, u = 0: the lowest id
