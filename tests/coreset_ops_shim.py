"""TEST-ONLY stand-in for the handful of cclip_hip.ops entries clip/coreset.py calls, on CPU tensors (the pattern of
tests/cpu_ops_shim.py), so that the host logic of `select_coreset` - the three forms of `labelled`, the seeding, the first
pick, the limits - runs in a container without a GPU.  The selection itself is tests/coreset_ref.py's fp32 restatement of the
kernel.  It is never importable from the product package."""
import numpy as np
import torch

import coreset_ref as R

SIMILARITY_TOPK_MAX_K = 64
_MASK = 0xFFFFFFFF


def coreset_blocks(N):
    return min(1024, (N + 63) // 64)


def _key(row):
    return 0 if row < 0 else (1 << 32) | (~row & _MASK)


def _row(keys):
    top = int(keys.max())
    return -1 if top == 0 else (~top) & _MASK


def kmeans_assign(x, c, **kw):
    s = x.double() @ c.double().t()
    best, assign = s.max(dim=1)
    return assign.to(torch.int32), best.float(), None


def similarity_topk(q, g, k):
    s = (q.double() @ g.double().t()).float()
    scores, index = torch.sort(s, dim=1, descending=True, stable=True)
    return scores[:, :k], index[:, :k].to(torch.int32)


def _w(weight):
    return None if weight is None else weight.numpy()


def coreset_step(x, mind, owner, partial_out, *, scan_only=False, weight=None, **kw):
    assert scan_only, "clip/coreset.py only scans through coreset_step"
    partial_out.zero_()
    partial_out[0] = _key(R.scan32(_w(weight), mind.numpy(), owner.numpy().astype(np.int64)))
    return None, None


def coreset_greedy(x, mind, owner, m, *, first=None, workspace=None, weight=None):
    X32 = x.float().numpy()
    md, ow = mind.numpy().copy(), owner.numpy().astype(np.int64)
    nxt = _row(workspace[0]) if first is None else int(first)
    picks, radius = [], []
    for _ in range(m):
        if nxt < 0:
            picks.append(-1); radius.append(float("nan"))
            continue
        md, ow, r = R.step32(X32, _w(weight), md, ow, nxt)
        picks.append(nxt); radius.append(float(r))
        nxt = R.scan32(_w(weight), md, ow)
    mind.copy_(torch.from_numpy(md))
    owner.copy_(torch.from_numpy(ow).to(torch.int32))
    return torch.tensor(picks, dtype=torch.int32), torch.tensor(radius, dtype=torch.float32), workspace
