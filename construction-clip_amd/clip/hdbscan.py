"""HDBSCAN over the stored embeddings: density clusters without a k, noise labelled as noise.

`kmeans` needs the number of clusters and places every photo; `duplicate_groups` is single linkage at one hand-picked
threshold.  HDBSCAN (Campello, Moulavi & Sander 2013, "Density-based clustering based on hierarchical density estimates")
sits between the two: single linkage at EVERY threshold, on a similarity that pushes sparse rows away, and the clusters that
persist longest are kept.

    s[i, j]  = <x_i, x_j>                                     the fp32 MFMA score of the stored unit 16-bit rows
    core[i]  = the min_samples-th largest s[i, .], the row itself counted (+inf for min_samples == 1)
    m[i, j]  = min(s[i, j], core[i], core[j])                 mutual-reachability similarity
    tree     = the maximum spanning tree of the complete graph under m, ties broken by (min(i, j), max(i, j))
    d        = sqrt(max(0, 2 - 2 m)),  lambda = 1 / max(d, 1e-6)       chord length: the Euclidean distance of unit rows

The tree is the O(N^2 D) part and runs on the device (csrc/mst.hip: Boruvka rounds enqueued by one native call, the N x N
matrix never written, integer atomics only, nothing read back).  Turning its N - 1 edges into clusters - the single-linkage
tree, the condensed tree, the stability selection - is O(N log N) pointer work and runs on the host in numpy; reading the
edges is the one host read.  Binary merges happen in the sorted edge order, so a result is a pure function of the edge list.
On unit rows the results are comparable with sklearn.cluster.HDBSCAN(metric="euclidean").
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np
import torch

from cclip_hip import ops
from .retrieval import EmbeddingIndex, connected_components
from .tsne import _unit_rows

LAMBDA_MIN_DISTANCE = 1e-6
SELECTIONS = ("eom", "leaf")


@dataclass
class MSTResult:
    """u, v int64 [N - 1]: the tree's edges, u < v, sorted by the total order (larger similarity first, then the smaller u,
    then the smaller v); similarity fp32 [N - 1]: their mutual-reachability similarity; distance fp32 [N - 1]: the
    chord length sqrt(max(0, 2 - 2 similarity)), ascending; core fp32 [N]: the core similarity of every row.  Tensors live on
    the device; N == 1 has no edges (and allows min_samples = 1 only)."""
    u: torch.Tensor
    v: torch.Tensor
    similarity: torch.Tensor
    distance: torch.Tensor
    core: torch.Tensor

    def __len__(self) -> int:
        return int(self.core.numel())

    def cut(self, threshold: float) -> torch.Tensor:
        """int64 [N] (host): the components of the tree edges with similarity >= threshold, every row labelled by the lowest
        row of its component.  With min_samples == 1 this is single linkage at that threshold: the partition
        `EmbeddingIndex.duplicate_groups(threshold)` yields."""
        keep = self.similarity >= float(threshold)
        return connected_components(len(self), torch.stack([self.u[keep], self.v[keep]], dim=1))


@dataclass
class HDBSCANResult:
    """labels int64 [N]: the cluster of every row, -1 = noise, clusters numbered by their lowest row; probabilities fp32 [N]:
    min(lambda of the row, lambda_max of its cluster) / lambda_max, 0 for noise; persistence fp32 [n_clusters]: the stability
    sum over the cluster's rows of (lambda - lambda at the cluster's birth); mst: the `MSTResult` underneath."""
    labels: torch.Tensor
    probabilities: torch.Tensor
    persistence: torch.Tensor
    n_clusters: int
    mst: MSTResult


def _count(features) -> int:
    if isinstance(features, EmbeddingIndex):
        return len(features)
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or not features.is_floating_point():
        raise ValueError(f"hdbscan: features must be an EmbeddingIndex or a 2-D float tensor, got "
                         f"{getattr(features, 'dtype', type(features))} {tuple(getattr(features, 'shape', ()))}")
    return int(features.shape[0])


def _check_min_samples(N: int, min_samples) -> int:
    if N < 1:
        raise ValueError("hdbscan: no rows")
    if isinstance(min_samples, bool) or int(min_samples) != min_samples:
        raise ValueError(f"hdbscan: min_samples = {min_samples!r} must be an integer")
    top = min(N, ops.SIMILARITY_TOPK_MAX_K)
    if not 1 <= min_samples <= top:
        raise ValueError(f"hdbscan: min_samples = {min_samples} outside [1, {top}] ({N} rows; the top-k kernel returns at most "
                         f"{ops.SIMILARITY_TOPK_MAX_K} entries)")
    return int(min_samples)


def _order_key(m: torch.Tensor) -> torch.Tensor:
    """int64 image of the kernels' score_key: larger = larger fp32, -0 == +0, NaN -> 0"""
    b = (m + 0.0).view(torch.int32).long()
    key = torch.where(b < 0, (~b) & 0xFFFFFFFF, (b & 0xFFFFFFFF) | 0x80000000)
    return torch.where(m != m, torch.zeros_like(key), key)


def chord(similarity: torch.Tensor) -> torch.Tensor:
    return (2.0 - 2.0 * similarity).clamp_(min=0.0).sqrt_()


@torch.no_grad()
def mutual_reachability_mst(features: Union[torch.Tensor, EmbeddingIndex], min_samples: int = 5,
                            dtype: Optional[torch.dtype] = None) -> MSTResult:
    """The maximum spanning tree of [N, E] features (any float dtype, anywhere: normalised and rounded to `dtype`, default
    bfloat16; 16-bit device rows are taken as unit rows as they are) or of an `EmbeddingIndex` (its stored rows, not copied)
    under mutual-reachability similarity at `min_samples` (1 .. min(N, 64); 1 = the plain similarity: the single-linkage
    tree; a single row needs min_samples = 1, the default 5 is a ValueError there as for any N < 5).  Everything stays on the
    device and nothing is read back.  Two calls return bitwise equal trees."""
    N = _count(features)
    min_samples = _check_min_samples(N, min_samples)
    x = _unit_rows(features, dtype)
    dev = x.device
    if min_samples == 1:
        core = torch.full((N,), float("inf"), device=dev, dtype=torch.float32)
    else:
        scores, _ = ops.similarity_topk(x, x, min_samples)
        core = scores[:, min_samples - 1].contiguous()
    u, v, m = ops.mst_boruvka(x, core)
    u, v = u.long(), v.long()
    lo, hi = torch.minimum(u, v), torch.maximum(u, v)
    key = torch.where(u < 0, torch.full_like(lo, -1), _order_key(m))          # the one empty slot goes last
    order = torch.argsort(hi, stable=True)
    order = order[torch.argsort(lo[order], stable=True)]
    order = order[torch.argsort(key[order], descending=True, stable=True)][:N - 1]
    sim = m[order]
    return MSTResult(u=lo[order], v=hi[order], similarity=sim, distance=chord(sim), core=core)      # u < v


# ---------------------------------------------------------------------------------------------------------------------------
# host side: N - 1 sorted edges -> clusters (numpy, float64)

def single_linkage(n: int, u, v) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The binary merge tree of n points from tree edges in merge order: edge k joins the nodes left[k] and right[k] into node
    n + k (points are 0 .. n - 1).  Returns (left, right, size [2 n - 1])."""
    top = np.arange(2 * n - 1, dtype=np.int64)            # union-find: the current node above every node
    left = np.empty(n - 1, dtype=np.int64)
    right = np.empty(n - 1, dtype=np.int64)
    size = np.ones(2 * n - 1, dtype=np.int64)

    def find(a: int) -> int:
        r = a
        while top[r] != r:
            r = top[r]
        while top[a] != r:
            top[a], a = r, top[a]
        return r

    for k in range(n - 1):
        a, b = find(int(u[k])), find(int(v[k]))
        if a == b:
            raise ValueError(f"hdbscan: edge {k} ({int(u[k])}, {int(v[k])}) closes a cycle: the edges are no spanning tree")
        node = n + k
        left[k], right[k] = a, b
        top[a] = top[b] = node
        size[node] = size[a] + size[b]
    return left, right, size


def _points_under(n: int, left, right, node: int):
    out, stack = [], [node]
    while stack:
        a = stack.pop()
        if a < n:
            out.append(a)
        else:
            stack.append(int(right[a - n]))
            stack.append(int(left[a - n]))
    return out


def condense_tree(n: int, left, right, size, lam, min_cluster_size: int):
    """The condensed tree as rows (parent, child, lambda, child size): clusters are numbered from n (the root) on, a child
    below n is a row that falls out of `parent` at `lambda`.  A split whose sides both hold min_cluster_size rows makes two
    new clusters; a smaller side falls out of the parent, which lives on in the other side."""
    rows = []
    if n < 2:
        return rows
    name = {2 * n - 2: n}
    nxt = n + 1
    stack = [2 * n - 2]
    while stack:
        node = stack.pop()
        k = node - n
        c, lv = name[node], float(lam[k])
        sides = (int(left[k]), int(right[k]))
        big = [s for s in sides if size[s] >= min_cluster_size]
        if len(big) == 2:
            for s in sides:
                name[s] = nxt
                rows.append((c, nxt, lv, int(size[s])))
                nxt += 1
                stack.append(s)
        else:
            for s in sides:
                if s in big:
                    name[s] = c
                    stack.append(s)
                else:
                    rows.extend((c, p, lv, 1) for p in _points_under(n, left, right, s))
    return rows


def select_clusters(n: int, rows, method: str, allow_single_cluster: bool):
    """(selected cluster ids, stability dict) from the condensed rows: "eom" keeps a cluster if its own stability is at least the
    sum of the best of its children, "leaf" keeps the leaves of the cluster tree.  The root is a candidate only with
    allow_single_cluster."""
    root = n
    birth = {root: 0.0}
    children = {root: []}
    for p, c, lv, sz in rows:
        if c >= n:
            birth[c] = lv
            children[c] = []
            children[p].append(c)
    stability = {c: 0.0 for c in children}
    for p, c, lv, sz in rows:
        stability[p] += (lv - birth[p]) * sz
    own = dict(stability)
    if method == "leaf":
        chosen = [c for c in children if not children[c] and (c != root or allow_single_cluster)]
        return sorted(chosen), own
    selected = {c: True for c in children}
    if not allow_single_cluster:
        selected[root] = False
    for c in sorted(children, reverse=True):                # children carry larger ids than their parent
        if c == root and not allow_single_cluster:
            continue
        below = sum(stability[k] for k in children[c])
        if below > stability[c]:
            selected[c] = False
            stability[c] = below
        else:
            stack = list(children[c])
            while stack:
                k = stack.pop()
                selected[k] = False
                stack.extend(children[k])
    return sorted(c for c in children if selected[c]), own


def tree_clusters(n: int, u, v, distance, min_cluster_size: int = 5, cluster_selection: str = "eom",
                  allow_single_cluster: bool = False):
    """Sorted tree edges (u, v, distance ascending; float64) -> (labels int64 [n], probabilities float64 [n], persistence
    float64 [clusters]).  The host half of `hdbscan`, usable on any spanning tree."""
    labels = np.full(n, -1, dtype=np.int64)
    prob = np.zeros(n, dtype=np.float64)
    if n == 1:
        if allow_single_cluster:
            labels[0], prob[0] = 0, 1.0
            return labels, prob, np.zeros(1)
        return labels, prob, np.zeros(0)
    d = np.asarray(distance, dtype=np.float64)
    lam = 1.0 / np.maximum(d, LAMBDA_MIN_DISTANCE)
    left, right, size = single_linkage(n, u, v)
    rows = condense_tree(n, left, right, size, lam, min_cluster_size)
    chosen, own = select_clusters(n, rows, cluster_selection, allow_single_cluster)
    chosen_set = set(chosen)
    above = {n: n if n in chosen_set else -1}              # the selected cluster at or above every cluster, -1 = none
    lam_max = {}
    for p, c, lv, sz in rows:                               # (a parent's row precedes the rows of its children)
        if c >= n:
            above[c] = c if c in chosen_set else above[p]
        lam_max[p] = max(lam_max.get(p, 0.0), lv)
    lowest = {}
    for p, c, lv, sz in rows:
        if c < n and above[p] >= 0:
            s = above[p]
            labels[c] = s
            prob[c] = min(lv, lam_max[s]) / lam_max[s]
            lowest[s] = min(lowest.get(s, n), c)
    order = sorted(lowest, key=lowest.get)                  # clusters numbered by their lowest row
    number = {s: i for i, s in enumerate(order)}
    labels = np.array([number[s] if s >= 0 else -1 for s in labels], dtype=np.int64)
    return labels, prob, np.array([own[s] for s in order], dtype=np.float64)


def _check_arguments(N: int, min_cluster_size, min_samples, cluster_selection):
    if isinstance(min_cluster_size, bool) or int(min_cluster_size) != min_cluster_size or min_cluster_size < 2:
        raise ValueError(f"hdbscan: min_cluster_size = {min_cluster_size!r} must be an integer >= 2")
    if cluster_selection not in SELECTIONS:
        raise ValueError(f"hdbscan: cluster_selection = {cluster_selection!r}; expected one of {SELECTIONS}")
    if N < 1:
        raise ValueError("hdbscan: no rows")
    if min_samples is None:
        min_samples = min(int(min_cluster_size), ops.SIMILARITY_TOPK_MAX_K, N)
    return int(min_cluster_size), _check_min_samples(N, min_samples)


@torch.no_grad()
def hdbscan(features: Union[torch.Tensor, EmbeddingIndex], min_cluster_size: int = 5, min_samples: Optional[int] = None,
            cluster_selection: str = "eom", allow_single_cluster: bool = False,
            dtype: Optional[torch.dtype] = None) -> HDBSCANResult:
    """HDBSCAN of [N, E] features or of an `EmbeddingIndex` (as for `mutual_reachability_mst`).  min_cluster_size >= 2: the
    fewest rows a cluster holds.  min_samples: the neighbour whose similarity is a row's core similarity, the row itself
    counted, 1 .. min(N, 64); None = min_cluster_size, capped at 64 and at N.  cluster_selection: "eom" (excess of mass) or
    "leaf".  allow_single_cluster: the whole set may come back as one cluster.

    The argument errors are raised before anything touches a device.  The tree is built on the device; its N - 1 edges are
    read once and the cluster tree is made on the host.  Two calls return equal results."""
    N = _count(features)
    min_cluster_size, min_samples = _check_arguments(N, min_cluster_size, min_samples, cluster_selection)
    mst = mutual_reachability_mst(features, min_samples, dtype)
    dev = mst.core.device
    edges = torch.stack([mst.u.double(), mst.v.double(), mst.similarity.double()]).cpu().numpy()      # the one host read
    d = np.sqrt(np.maximum(0.0, 2.0 - 2.0 * edges[2]))
    labels, prob, pers = tree_clusters(N, edges[0].astype(np.int64), edges[1].astype(np.int64), d, min_cluster_size,
                                       cluster_selection, allow_single_cluster)
    return HDBSCANResult(labels=torch.from_numpy(labels).to(dev), probabilities=torch.from_numpy(prob).float().to(dev),
                         persistence=torch.from_numpy(pers).float().to(dev), n_clusters=int(pers.shape[0]), mst=mst)
