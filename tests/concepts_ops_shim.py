"""TEST-ONLY stand-in for the cclip_hip.ops entries clip/concepts.py calls, on CPU tensors (the pattern of
tests/coreset_ops_shim.py), so that the host logic of `decompose` - chunking, truncation, centring, the profile - runs in a
container without a GPU.  The codes themselves are tests/concepts_ref.py's fp32 restatement.  It is never importable from the
product package."""
import numpy as np
import torch

import concepts_ref as R

CALLS = []                                                 # (rows, V) of every concept_codes call: the chunking tests read it


def concept_codes_workspace(N, V, D):
    return 4 * N * ((V + 3) // 4 * 4)


def concept_codes(x, c, l1, eta, iters, *, out_w=None, workspace=None):
    N, V = x.shape[0], c.shape[0]
    CALLS.append((N, V))
    if workspace is not None:
        assert workspace.numel() * 4 >= concept_codes_workspace(N, V, x.shape[1])
    # row by row, as the kernel's rows are independent of N and of their position (a batched BLAS product is not, bit for bit)
    X, C = x.float().numpy(), c.float().numpy()
    per_row = [R.fista32(X[i:i + 1], C, l1, eta, iters) for i in range(N)]
    o = {k: np.concatenate([p[k] for p in per_row]) for k in ("w", "resid2", "l1norm", "nnz", "delta", "kkt")}
    w = torch.from_numpy(o["w"])
    if out_w is None:
        out_w = w
    else:
        assert tuple(out_w.shape) == (N, V) and out_w.dtype == torch.float32
        out_w.copy_(w)
    f = lambda k, dt: torch.from_numpy(o[k]).to(dt)        # noqa: E731
    return out_w, f("resid2", torch.float32), f("l1norm", torch.float32), f("nnz", torch.int32), f("delta", torch.float32), \
        f("kkt", torch.float32)
