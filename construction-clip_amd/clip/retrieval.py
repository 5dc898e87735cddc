"""Retrieval over stored embeddings: "which photos match this description / this photo?" and recall@k.

The reference stops at the embedding pickle (CLIP_prefix_caption/parse_coco.py) and an in-batch accuracy among 8
(CLIP/train_caption.py:124-136).  `EmbeddingIndex` keeps the L2-normalised rows on the device in the 16-bit type the towers
compute in and answers a batch of queries with the fused similarity top-k kernel (csrc/embed_topk.hip): exact, the Q x N
score matrix is never formed, no host read.  `retrieval_recall` is the usual image <-> text R@k on top of it.

The fixed-radius query (csrc/embed_range.hip) is the other half: `range_search` returns every stored row above a similarity,
`duplicate_pairs` / `duplicate_groups` find the repeated photos of a set (the reference's monthly reports re-use them), and
`group_split` holds out whole groups, so that no validation row has a twin on the training side.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from cclip_hip import ops

HALF_TYPES = (torch.bfloat16, torch.float16)


def _device(t: Optional[torch.Tensor] = None) -> torch.device:
    if t is not None and t.is_cuda:
        return t.device
    return torch.device("cuda", torch.cuda.current_device())


def normalize_rows(features: torch.Tensor, dtype: torch.dtype, device: Optional[torch.device] = None) -> torch.Tensor:
    """[N, E] of any float dtype, anywhere -> device rows L2-normalised in fp32 (cclip_l2norm_fwd), then rounded to `dtype`."""
    if features.dim() != 2 or not features.is_floating_point():
        raise ValueError(f"expected a 2-D float tensor of features, got {tuple(features.shape)} {features.dtype}")
    if dtype not in HALF_TYPES:
        raise ValueError(f"dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    dev = device if device is not None else _device(features)
    x = features.detach().to(device=dev, dtype=torch.float32).contiguous()
    N, E = x.shape
    out = torch.empty(N, E, device=dev, dtype=dtype)
    if N == 0:
        return out
    y = torch.empty_like(x)
    inv = torch.empty(N, device=dev, dtype=torch.float32)
    ops.l2norm_fwd(x, y, inv)
    ops.cast_f32_to_bf16(y, out)
    return out


class EmbeddingIndex:
    """Stored embeddings [N, E] on the device, searchable.  `metadata`: an optional list of N entries (the embedding pickle's
    `captions` dicts carry `file_name`).  `dtype`: the 16-bit type of the stored rows and of the queries (default bfloat16,
    pass `model.compute_dtype` to match a model)."""

    def __init__(self, features: torch.Tensor, dtype: Optional[torch.dtype] = None, metadata: Optional[Sequence] = None):
        self.dtype = torch.bfloat16 if dtype is None else dtype
        rows = normalize_rows(features, self.dtype)
        if rows.shape[1] % 32 or rows.shape[1] > ops.SIMILARITY_TOPK_MAX_D:
            raise NotImplementedError(f"EmbeddingIndex: embedding width {rows.shape[1]}; the search kernel needs a multiple of 32 "
                                      f"up to {ops.SIMILARITY_TOPK_MAX_D}")
        if metadata is not None and len(metadata) != rows.shape[0]:
            raise ValueError(f"metadata has {len(metadata)} entries for {rows.shape[0]} rows")
        self._buf = rows                     # capacity rows; the first _n are live
        self._n = rows.shape[0]
        self.metadata = None if metadata is None else list(metadata)

    def __len__(self) -> int:
        return self._n

    @property
    def dim(self) -> int:
        return self._buf.shape[1]

    @property
    def features(self) -> torch.Tensor:
        """The stored normalised 16-bit rows [N, E] (a view)."""
        return self._buf[:self._n]

    def add(self, features: torch.Tensor, metadata: Optional[Sequence] = None) -> "EmbeddingIndex":
        """Append rows (amortised growth: capacity doubles).  Rows are normalised one by one, so the stored bits equal a bulk build's."""
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError(f"add: expected [*, {self.dim}] features, got {tuple(features.shape)}")
        if (metadata is None) != (self.metadata is None) and self._n > 0:
            raise ValueError("add: metadata must be given for every row of the index or for none")
        if metadata is not None and len(metadata) != features.shape[0]:
            raise ValueError(f"add: metadata has {len(metadata)} entries for {features.shape[0]} rows")
        rows = normalize_rows(features, self.dtype, self._buf.device)
        need = self._n + rows.shape[0]
        if need > self._buf.shape[0]:
            grown = torch.empty(max(need, 2 * self._buf.shape[0]), self.dim, device=self._buf.device, dtype=self.dtype)
            grown[:self._n].copy_(self._buf[:self._n])
            self._buf = grown
        self._buf[self._n:need].copy_(rows)
        self._n = need
        if metadata is not None:
            self.metadata = (self.metadata or []) + list(metadata)
        return self

    @classmethod
    def from_pickle(cls, path: str, dtype: Optional[torch.dtype] = None) -> "EmbeddingIndex":
        """The embedding file of clip_caption.data.save_embeddings / scripts/extract_embeddings.py (parse_coco.py's layout):
        row captions[i]["clip_embedding"] of `clip_embedding` belongs to captions[i]."""
        from clip_caption.data import load_embeddings
        data = load_embeddings(path)
        emb, captions = data["clip_embedding"], data["captions"]
        order = [int(c["clip_embedding"]) if isinstance(c, dict) and "clip_embedding" in c else i for i, c in enumerate(captions)]
        if order != list(range(emb.shape[0])):
            emb = emb[torch.tensor(order, dtype=torch.long)]
        return cls(emb, dtype=dtype, metadata=captions)

    @torch.no_grad()
    def search(self, queries: torch.Tensor, k: int = 10, *, querybank=None, mask: Optional[torch.Tensor] = None,
               return_gate: bool = False):
        """queries [Q, E] (any float dtype, anywhere) -> (scores fp32 [Q, k] descending, indices int64 [Q, k]) on the device:
        cosine similarity of the normalised 16-bit rows, equal scores by the lower index.

        querybank: a `QueryBank` (`self.querybank(bank)`, clip/hubness.py) ranks by the hubness-corrected value
        fmaf(scale, cosine, bias[row]) instead and returns those values; with method "dis" only the queries whose raw best row
        is in the bank's activation set do, every other query keeps its raw result bit for bit.  A bank fitted at another
        len(index) raises ValueError.  mask: bool [N], True = leave the row out (filtered search: `labels != wanted`); such a
        row can only appear once the other rows run out (k above their number), with score -inf.  return_gate appends a bool
        [Q]: the queries that took the normalised path.  Without a keyword the call is the plain top-k, as ever."""
        if self._n == 0:
            raise ValueError("search: the index is empty")
        if queries.dim() == 1:
            queries = queries[None]
        if queries.dim() != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"search: expected [*, {self.dim}] queries, got {tuple(queries.shape)}")
        q = normalize_rows(queries, self.dtype, self._buf.device)
        if querybank is None and mask is None:
            scores, index = ops.similarity_topk(q, self.features, int(k))
            gate = torch.zeros(q.shape[0], device=q.device, dtype=torch.bool) if return_gate else None
        else:
            from .hubness import corrected_topk
            scores, index, gate = corrected_topk(q, self.features, int(k), querybank, mask)
        return (scores, index.long(), gate) if return_gate else (scores, index.long())

    def querybank(self, bank: torch.Tensor, **kw):
        """A `QueryBank` for the rows stored now (clip/hubness.py: csrc/embed_hub.hip), from `bank` [B, E], a sample of typical
        queries: method "dis" (default), "is" or "csls", beta, k, activation_k.  Fit it again after `add`."""
        from .hubness import fit_querybank
        return fit_querybank(self, bank, **kw)

    @torch.no_grad()
    def range_search(self, queries: torch.Tensor, threshold: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """queries [Q, E] (normalised exactly as `search` does) -> (offsets int64 [Q+1], indices int64 [H], scores fp32 [H]) on
        the device: every stored row with cosine similarity >= threshold, the rows of query i in ascending index order at
        offsets[i] .. offsets[i+1].  The fixed-radius query (csrc/embed_range.hip); the Q x N matrix is never formed.  One
        host read (the total H sizes the outputs)."""
        if self._n == 0:
            raise ValueError("range_search: the index is empty")
        if queries.dim() == 1:
            queries = queries[None]
        if queries.dim() != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"range_search: expected [*, {self.dim}] queries, got {tuple(queries.shape)}")
        q = normalize_rows(queries, self.dtype, self._buf.device)
        offsets, index, scores = ops.similarity_range(q, self.features, float(threshold))
        return offsets, index.long(), scores

    @torch.no_grad()
    def duplicate_pairs(self, threshold: float = 0.95) -> Tuple[torch.Tensor, torch.Tensor]:
        """Near-duplicates among the stored rows: (pairs int64 [P, 2], scores fp32 [P]) on the device, every i < j with cosine
        similarity >= threshold, sorted by i, then j (the kernel's self-join order: nothing is sorted here).  An empty index
        has no pairs."""
        dev = self._buf.device
        if self._n == 0:
            return torch.empty(0, 2, device=dev, dtype=torch.int64), torch.empty(0, device=dev, dtype=torch.float32)
        rows = self.features
        offsets, index, scores = ops.similarity_range(rows, rows, float(threshold), self_join=True)
        first = torch.repeat_interleave(torch.arange(self._n, device=dev), offsets.diff(), output_size=index.numel())
        return torch.stack([first, index.long()], dim=1), scores

    @torch.no_grad()
    def duplicate_groups(self, threshold: float = 0.95) -> torch.Tensor:
        """Single-linkage groups of near-duplicates: int64 [N] (host), the connected components of the `duplicate_pairs`
        graph, every row labelled by the smallest row index of its group - a row without a duplicate by itself."""
        pairs, _ = self.duplicate_pairs(threshold)
        return connected_components(self._n, pairs)

    def kmeans(self, k: int, **kw):
        """Spherical k-means of the stored rows (clip/cluster.py: csrc/embed_kmeans.hip): a `KMeansResult`.  The rows are used
        as stored, not copied."""
        from .cluster import kmeans
        return kmeans(self, k, **kw)

    @torch.no_grad()
    def assign(self, centroids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Place the stored rows into existing clusters: centroids [k, E] (a `KMeansResult.centroids`, or any float rows, which
        are normalised as `search` normalises queries) -> (labels int64 [N], scores fp32 [N]) on the device, the nearest
        centroid of every row by cosine similarity, equal scores by the lower centroid."""
        if self._n == 0:
            raise ValueError("assign: the index is empty")
        if centroids.dim() != 2 or centroids.shape[1] != self.dim or centroids.shape[0] < 1:
            raise ValueError(f"assign: expected [k >= 1, {self.dim}] centroids, got {tuple(centroids.shape)}")
        from .cluster import _rows16
        labels, scores, _ = ops.kmeans_assign(self.features, _rows16(centroids, self.dtype, self._buf.device))
        return labels.long(), scores

    @torch.no_grad()
    def knn_graph(self, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scores fp32 [N, k], index int32 [N, k]) on the device: the k most similar OTHER stored rows of every stored row,
        best first (clip/tsne.py: the top k + 1 of the self-join without the row itself, hence k <= 63).  No host read."""
        if self._n == 0:
            raise ValueError("knn_graph: the index is empty")
        from .tsne import knn_graph
        return knn_graph(self.features, k)

    def tsne(self, **kw):
        """A 2-D t-SNE map of the stored rows (clip/tsne.py: csrc/tsne.hip): a `TSNEResult`."""
        from .tsne import tsne
        return tsne(self, **kw)

    def spread_labels(self, labels, **kw):
        """Spread the labels of a few stored rows over the kNN graph (clip/propagate.py: csrc/label_spread.hip): labels, N
        integers with a value below 0 for an unlabelled row -> a `LabelSpreadResult`."""
        from .propagate import spread_labels
        return spread_labels(self, labels, **kw)

    def coreset(self, m: int, **kw):
        """k-centre greedy selection of m stored rows, from the labelled ones if any (clip/coreset.py: csrc/coreset.hip): a
        `CoresetResult`.  The rows are used as stored, not copied."""
        from .coreset import select_coreset
        return select_coreset(self, m, **kw)

    def mst(self, min_samples: int = 5):
        """The maximum spanning tree of the stored rows under mutual-reachability similarity (clip/hdbscan.py: csrc/mst.hip):
        an `MSTResult`.  The rows are used as stored, not copied."""
        from .hdbscan import mutual_reachability_mst
        return mutual_reachability_mst(self, min_samples)

    def hdbscan(self, **kw):
        """HDBSCAN of the stored rows: density clusters without a k, noise labelled -1 (clip/hdbscan.py): an `HDBSCANResult`."""
        from .hdbscan import hdbscan
        return hdbscan(self, **kw)

    def decompose(self, dictionary, **kw):
        """The stored rows as sparse non-negative combinations of a `ConceptDictionary`'s concepts (clip/concepts.py:
        csrc/concept_codes.hip): a `ConceptDecomposition`.  The rows are used as stored, not copied, unless centred."""
        from .concepts import decompose
        return decompose(self, dictionary, **kw)

    def gaussian(self, key: str, **kw):
        """A `GaussianClassifier` fitted on the stored rows with the labels the metadata carries under `key`
        (clip/gaussian.py: csrc/embed_moments.hip, csrc/gauss_scores.hip).  The rows are used as stored, not copied."""
        from .gaussian import GaussianClassifier
        return GaussianClassifier.from_index(self, key, **kw)

    def pca(self, k: int, **kw):
        """The k leading principal components of the stored rows (clip/gaussian.py): a `PCAResult`."""
        from .gaussian import pca
        return pca(self, k, **kw)

    @torch.no_grad()
    def search_text(self, model, tokens: torch.Tensor, k: int = 10, **kw):
        return self.search(model.encode_text(tokens.to(self._buf.device)), k, **kw)

    @torch.no_grad()
    def search_image(self, model, images: torch.Tensor, k: int = 10, **kw):
        return self.search(model.encode_image(images.to(self._buf.device)), k, **kw)


def connected_components(n: int, pairs: torch.Tensor) -> torch.Tensor:
    """Labels int64 [n] (host) of the graph on rows 0 .. n-1 with the edges pairs [P, 2]: every row carries the smallest row
    index of its component.  Union-find on the host: the smaller root always wins, so a root is its component's minimum."""
    parent = list(range(n))

    def find(x: int) -> int:
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:                 # path compression
            parent[x], x = root, parent[x]
        return root

    for a, b in pairs.cpu().tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return torch.tensor([find(x) for x in range(n)], dtype=torch.int64)


def group_split(groups: torch.Tensor, val_fraction: float, seed: int) -> Tuple[list, list]:
    """Split rows into (train_idx, val_idx), both sorted lists, without cutting a group: groups int64 [N] gives every row's
    group label (`EmbeddingIndex.duplicate_groups`).  The groups, in ascending label order, are drawn in the order of
    torch.randperm(number of groups) seeded with `seed`, and moved whole to the validation side until it holds at least
    max(1, round(val_fraction N)) rows; the last group always stays on the training side.  With every group of size 1
    (labels 0 .. N-1) and the same seed this is exactly the split scripts/train_caption.py --val-fraction makes without
    groups: the first min(N - 1, max(1, round(val_fraction N))) rows of the seeded row permutation."""
    groups = torch.as_tensor(groups).cpu()
    if groups.dim() != 1 or groups.numel() == 0 or groups.is_floating_point():
        raise ValueError(f"group_split: expected one integer group label per row, got {tuple(groups.shape)} {groups.dtype}")
    if not val_fraction > 0:
        raise ValueError(f"group_split: val_fraction = {val_fraction} must be positive")
    N = groups.numel()
    labels, member = torch.unique(groups, sorted=True, return_inverse=True)
    G = labels.numel()
    if G < 2:
        raise ValueError("group_split: all rows form one group; nothing can be held out")
    rows_of = [[] for _ in range(G)]
    for row, grp in enumerate(member.tolist()):
        rows_of[grp].append(row)
    perm = torch.randperm(G, generator=torch.Generator().manual_seed(int(seed))).tolist()
    want = max(1, int(round(val_fraction * N)))
    val = []
    for grp in perm[:G - 1]:
        if len(val) >= want:
            break
        val.extend(rows_of[grp])
    held = set(val)
    return [r for r in range(N) if r not in held], sorted(val)


def recall_from_indices(indices: torch.Tensor, query_labels: torch.Tensor, gallery_labels: torch.Tensor,
                        ks: Sequence[int]) -> torch.Tensor:
    """The hit rule: indices [Q, K] (best first) -> for each k in ks the share of queries with a gallery item of the query's
    label among their first k hits.  A [len(ks)] float64 tensor on indices' device; no host read."""
    Q, K = indices.shape
    if query_labels.shape != (Q,):
        raise ValueError(f"query_labels: expected [{Q}], got {tuple(query_labels.shape)}")
    if gallery_labels.dim() != 1:
        raise ValueError(f"gallery_labels: expected one label per gallery row, got {tuple(gallery_labels.shape)}")
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1 or max(ks) > K:
        raise ValueError(f"ks = {ks} must lie in 1 .. {K}")
    dev = indices.device
    hit = gallery_labels.to(dev)[indices.long()] == query_labels.to(dev)[:, None]          # [Q, K]
    first = torch.where(hit.any(dim=1), hit.to(torch.int64).argmax(dim=1), torch.full((Q,), K, device=dev, dtype=torch.int64))
    kk = torch.tensor(ks, device=dev, dtype=torch.int64)
    return (first[None, :] < kk[:, None]).to(torch.float64).mean(dim=1)


@torch.no_grad()
def retrieval_recall(query_features: torch.Tensor, gallery_features: torch.Tensor, ks: Sequence[int] = (1, 5, 10),
                     query_labels: Optional[torch.Tensor] = None, gallery_labels: Optional[torch.Tensor] = None,
                     dtype: Optional[torch.dtype] = None, bank_features: Optional[torch.Tensor] = None,
                     **querybank_kw) -> Dict[int, float]:
    """Recall@k of retrieving `gallery_features` rows with `query_features` rows: the share of queries whose top k holds a
    gallery item with the query's label.  Default labels pair query i with gallery row i (needs Q == N); pass labels when
    several gallery rows answer one query (the reference's data repeats `violation_list` strings).  One search at max(ks),
    the hit test on the device, one read-back of len(ks) numbers.  Every k must be <= min(64, N).  bank_features [B, E]: a
    sample of typical queries; the search is then the hubness-corrected one of `EmbeddingIndex.querybank(bank_features,
    **querybank_kw)` (method, beta, k, activation_k: clip/hubness.py)."""
    Q, N = query_features.shape[0], gallery_features.shape[0]
    if (query_labels is None) != (gallery_labels is None):
        raise ValueError("retrieval_recall: give both query_labels and gallery_labels, or neither")
    if query_labels is None:
        if Q != N:
            raise ValueError(f"retrieval_recall: without labels query i pairs with gallery row i, but Q = {Q} and N = {N}")
        query_labels = torch.arange(Q)
        gallery_labels = torch.arange(N)
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1 or max(ks) > min(N, ops.SIMILARITY_TOPK_MAX_K):
        raise ValueError(f"retrieval_recall: ks = {ks} must lie in 1 .. min(N, {ops.SIMILARITY_TOPK_MAX_K}) = "
                         f"{min(N, ops.SIMILARITY_TOPK_MAX_K)}")
    if tuple(gallery_labels.shape) != (N,) or tuple(query_labels.shape) != (Q,):
        raise ValueError(f"retrieval_recall: labels must be [{Q}] and [{N}], got {tuple(query_labels.shape)} and "
                         f"{tuple(gallery_labels.shape)}")
    if bank_features is None and querybank_kw:
        raise ValueError(f"retrieval_recall: {sorted(querybank_kw)} need bank_features")
    index = EmbeddingIndex(gallery_features, dtype=dtype)
    querybank = None if bank_features is None else index.querybank(bank_features, **querybank_kw)
    _, idx = index.search(query_features, max(ks), querybank=querybank)
    r = recall_from_indices(idx, query_labels, gallery_labels, ks).tolist()
    return {k: v for k, v in zip(ks, r)}
