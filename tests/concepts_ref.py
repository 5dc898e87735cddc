"""Float64 restatement of the concept-code contract (include/cclip_hip.h, cclip_concept_codes; csrc/concept_codes.hip's header)
and an fp32 restatement of the same recurrence.  Per row, FISTA with the non-negative soft threshold, a fixed iteration count
and beta_k = k / (k + 3):

    y = w_k + beta_k (w_k - w_{k-1});   r = x - y C;   g = r C^T;   w_{k+1} = max(0, y + eta (g - l1))      (w_0 = w_{-1} = 0)

and the read-outs at w_T itself.  Nothing here is taken from the kernel: the tests pin this file by the KKT conditions and by
closed forms."""
import numpy as np
import torch


def unit_rows16(n, d, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    return torch.nn.functional.normalize(x, dim=1).to(dtype)


def rows64(t16):
    return t16.double().numpy()


def lipschitz(C):
    """the largest eigenvalue of C^T C, in float64 on the D x D Gram matrix"""
    C = np.asarray(C, dtype=np.float64)
    return float(np.linalg.eigvalsh(C.T @ C)[-1])


def readouts(X, C, w, w_prev, l1):
    r = X - w @ C
    g = r @ C.T
    over = g - l1
    viol = np.where(w > 0, np.abs(over), np.maximum(over, 0))
    return dict(resid2=(r * r).sum(1), l1norm=w.sum(1), nnz=(w > 0).sum(1), delta=np.abs(w - w_prev).max(1), kkt=viol.max(1),
                g=g)


def _fista(X, C, l1, eta, iters, ft):
    X, C = np.asarray(X, dtype=ft), np.asarray(C, dtype=ft)
    l1, eta = ft(l1), ft(eta)
    w = np.zeros((X.shape[0], C.shape[0]), dtype=ft)
    wp = w.copy()
    for k in range(iters):
        beta = ft(k) / ft(k + 3)
        y = w + beta * (w - wp)
        r = X - y @ C
        g = r @ C.T
        wp, w = w, np.maximum(ft(0), y + eta * (g - l1))
    out = readouts(X, C, w, wp, l1)
    out.update(w=w, w_prev=wp)
    return out


def fista64(X, C, l1, eta, iters):
    return _fista(X, C, l1, eta, iters, np.float64)


def fista32(X, C, l1, eta, iters):
    return _fista(X, C, l1, eta, iters, np.float32)


def planted(V, D, rows, seed, dtype=torch.bfloat16, shared=0.0):
    """(x16 [rows, D], c16 [V, D], pairs [rows, 2]): rows normalise(0.7 c_a + 0.5 c_b) over a random unit dictionary; with
    shared > 0 the dictionary is normalise(shared * s + noise) for one unit direction s (a correlated dictionary)."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.nn.functional.normalize(torch.randn(V, D, generator=g, dtype=torch.float64), dim=1)
    if shared:
        s = torch.nn.functional.normalize(torch.randn(1, D, generator=g, dtype=torch.float64), dim=1)
        noise = torch.nn.functional.normalize(shared * s + noise, dim=1)
    c16 = noise.to(dtype)
    pairs = torch.stack([torch.randperm(V, generator=g)[:2] for _ in range(rows)])
    c = c16.double()
    x = torch.nn.functional.normalize(0.7 * c[pairs[:, 0]] + 0.5 * c[pairs[:, 1]], dim=1)
    return x.to(dtype), c16, pairs.numpy()
