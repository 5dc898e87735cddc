"""Thin torch-tensor -> raw-pointer shims over the C ABI (include/cclip_hip.h).

torch is plumbing here: it owns device memory and the stream; every FLOP happens in
libcclip_hip.so.  All functions enqueue on torch's current stream and return immediately.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from ._lib import lib, check

c_void_p, c_int, c_long, c_float = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float

ACT_NONE, ACT_QUICKGELU, ACT_TANH, ACT_GELU_NEW, ACT_RELU = 0, 1, 2, 3, 4
ACT_DQUICKGELU, ACT_DTANH, ACT_DGELU_NEW, ACT_DRELU = 16, 17, 18, 19


# Optional per-launch timing of the dominant kernel family (bench.py's roofline leg): when GEMM_EVENTS is a
# list, every cclip_gemm_bf16 launch is bracketed by HIP events on the launch stream and
# (start, end, flops, layout) is appended.  None (default) = zero overhead.
GEMM_EVENTS = None


def _stream() -> c_void_p:
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]) -> c_void_p:
    return c_void_p(0 if t is None else t.data_ptr())


def _req(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype or not t.is_cuda:
        raise TypeError(f"{name}: expected cuda {dtype}, got {t.device} {t.dtype}")


HALF_TYPES = (torch.bfloat16, torch.float16)


def _req16(t: torch.Tensor, name: str):
    if t.dtype not in HALF_TYPES or not t.is_cuda:
        raise TypeError(f"{name}: expected cuda bfloat16/float16, got {t.device} {t.dtype}")


def _fn(base: str, *tensors):
    """Pick the bf16 or the fp16 twin of an entry point from the dtype of its 16-bit tensors (which must agree)."""
    kinds = {t.dtype for t in tensors if t is not None and t.dtype in HALF_TYPES}
    if len(kinds) > 1:
        raise TypeError(f"{base}: mixed bfloat16 / float16 operands")
    f16 = kinds == {torch.float16}
    if base == "cclip_gemm_bf16":
        return lib.cclip_gemm_f16 if f16 else lib.cclip_gemm_bf16
    if base == "cclip_cast_f32_to_bf16":
        return lib.cclip_cast_f32_to_f16 if f16 else lib.cclip_cast_f32_to_bf16
    return getattr(lib, base + "_f16") if f16 else getattr(lib, base)


def _is16(t) -> int:
    return int(t is not None and t.dtype in HALF_TYPES)


class GemmDesc(ctypes.Structure):
    _fields_ = [
        ("A", c_void_p), ("B", c_void_p),
        ("a_kcontig", c_int), ("b_kcontig", c_int),
        ("lda", c_long), ("ldb", c_long),
        ("M", c_int), ("N", c_int), ("K", c_int),
        ("alpha", c_float),
        ("bias", c_void_p),
        ("act", c_int),
        ("aux", c_void_p), ("ldaux", c_long),
        ("residual", c_void_p), ("ldr", c_long),
        ("out_f32", c_void_p), ("out_bf16", c_void_p), ("out_pre_bf16", c_void_p), ("ldc", c_long),
        ("split_k", c_int), ("split_ws", c_void_p),
        ("tile_config", c_int),
        ("colsum_out", c_void_p), ("colsum_accumulate", c_int), ("colsum_of_b", c_int),
        ("ln_stats", c_void_p), ("ln_c1", c_void_p), ("rowstats_out", c_void_p),
    ]


# Tile-configuration autotuner.  The GEMM tile configurations (128x128, 256x128, 256x256, persistent 256x128 with a
# streamed epilogue - forward layout / full tiles only) win on different
# shapes (tile-count quantisation over 256 CUs, K length, epilogue weight), and a model issues ~20 distinct GEMM
# shapes thousands of times.  The choice per (shape, layout, epilogue, split) key comes from a PERSISTED table:
#   * `gemm_tune.json` next to libcclip_hip.so (committed; refreshed by tools/tune_gemm.py on a GPU box), or the file named
#     by CCLIP_TUNE_FILE, is loaded at the first GEMM call.  It is keyed by a hash of the GEMM kernel sources: a table made
#     for other kernels is ignored.
#   * only a key the table does not hold is timed (trial launches on scratch outputs, GPU to itself), added to the table,
#     and - when CCLIP_TUNE_FILE is set or CCLIP_TUNE_SAVE=1 - written back, so the next process does not tune at all.
#   * under data parallelism rank 0's table is broadcast (`sync_tuned_table`), and a key missed later is decided by rank 0
#     for everyone: all ranks run the same tiles, hence the same summation order.
# With a complete table a run is launch-for-launch reproducible: no trial launches, no timing-dependent choices.
# AUTOTUNE=False pins configuration 1.
AUTOTUNE = True


class _GenDict(dict):
    """dict that counts its mutations (the per-family index of _nearest_tuned is rebuilt when the count moves)"""
    gen = 0

    def _bump(self):
        self.gen += 1

    def __setitem__(self, k, v):
        self._bump(); dict.__setitem__(self, k, v)

    def __delitem__(self, k):
        self._bump(); dict.__delitem__(self, k)

    def clear(self):
        self._bump(); dict.clear(self)

    def update(self, *a, **kw):
        self._bump(); dict.update(self, *a, **kw)

    def pop(self, *a):
        self._bump(); return dict.pop(self, *a)


_TUNED = _GenDict()        # timed / persisted entries ONLY (choices derived by _nearest_tuned live in _DERIVED)
_TUNE_MIN_FLOPS = 2.0 * (1 << 29)
_TUNE_STATE = {"loaded": False, "source_hash": None, "misses": 0, "path": None}


def _tune_paths():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    return os.environ.get("CCLIP_TUNE_FILE"), os.path.join(here, "gemm_tune.json")


def kernel_source_hash() -> str:
    """sha256 over the tile-GEMM kernel sources (csrc/gemm_bf16*.hip and the generated K loops gemm_a4*.inc, except the skinny GEMV path and the fp8 kernels, neither of
    which has tile configurations to choose from; gemm_bf16_impl.h, cclip_common.h): the key a tuned table is valid for."""
    import hashlib, os
    if _TUNE_STATE["source_hash"] is None:
        csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
        h = hashlib.sha256()
        for f in sorted(os.listdir(csrc)):
            if ((f.startswith("gemm_bf16") or f.startswith("gemm_a4")) and "skinny" not in f and "fp8" not in f) or f == "cclip_common.h":
                h.update(f.encode())
                with open(os.path.join(csrc, f), "rb") as fh:
                    h.update(fh.read())
        _TUNE_STATE["source_hash"] = h.hexdigest()[:16]
    return _TUNE_STATE["source_hash"]


import os as _os
_CFG_REMAP = {int(a): int(b) for a, b in (kv.split(":") for kv in _os.environ.get("CCLIP_GEMM_REMAP", "").split(",") if kv)}
class _LRU(dict):
    """bounded key -> choice cache of derived tile choices (insertion-ordered dict: oldest entry evicted first)"""
    cap = 1024

    def put(self, k, v):
        if k in self:
            dict.pop(self, k)
        elif len(self) >= self.cap:
            dict.pop(self, next(iter(self)))
        dict.__setitem__(self, k, v)

    def update(self, other=()):                     # accepts a dict or an iterable of keys (tests restore a saved key set)
        for k in other:
            self.put(k, other[k] if isinstance(other, dict) else None)


_DERIVED = _LRU()     # choices filled in by _nearest_tuned for keys the table does not hold: bounded, never persisted, never searched
_FAMILY = {"gen": -1, "idx": {}}


def _key_str(key) -> str:
    return "|".join(str(int(k)) if isinstance(k, bool) else str(k) for k in key)


def _family_of(f):
    """(family key, token field index, token count) of a split key: the family is the key with its TOKEN dimension blanked -
    rows of a forward-layout GEMM, the contraction length of a weight-gradient GEMM."""
    tok = 3 if (f[4] == "0" and f[5] == "0") else 1
    return "|".join(f[:tok] + ["*"] + f[tok + 1:]), tok, int(f[tok])


def _family_index():
    """family key -> (sorted token counts, choices in that order), built from the timed / persisted entries and rebuilt only
    when _TUNED changed.  A lookup is then one split of the QUERY key and a bisect: it does not grow with the number of keys a
    run has met (round 2 scanned - and string-split - every table entry per miss and stored derived entries in the same table,
    so a run with a new packed row count every step slowed down linearly with its length)."""
    if _FAMILY["gen"] != _TUNED.gen:
        fam = {}
        for k, v in _TUNED.items():
            fk, _, t = _family_of(k.split("|"))
            fam.setdefault(fk, []).append((t, v))
        _FAMILY["idx"] = {fk: ([t for t, _ in sorted(lst)], [v for _, v in sorted(lst)]) for fk, lst in fam.items()}
        _FAMILY["gen"] = _TUNED.gen
    return _FAMILY["idx"]


def _nearest_tuned(key: str, unbounded: bool = False):
    """A shape the table does not hold whose only difference from a tuned one is its TOKEN dimension (within 16x) - a last partial
    batch, a packed text batch whose row count follows the captions' lengths - takes that entry's tile configuration instead of
    being timed in the middle of the step: deterministic (no timing), no synchronisation.  A weight gradient's split-K count is
    scaled with the contraction length (same K-tiles per split).  `unbounded`: no distance limit (data parallelism: a rank must
    never time a shape on its own, see gemm_bf16).  CCLIP_TUNE_EXACT=1 (tools/tune_gemm.sh) disables it: every shape is timed."""
    import bisect, math, os
    if os.environ.get("CCLIP_TUNE_EXACT") == "1":
        return None
    fk, tok, want = _family_of(key.split("|"))
    ent = _family_index().get(fk)
    if ent is None:
        return None
    toks, vals = ent
    i = bisect.bisect_left(toks, want)
    best, best_d = None, (float("inf") if unbounded else math.log(16.0))
    for j in (i - 1, i):
        if 0 <= j < len(toks):
            d = abs(math.log(toks[j] / want))
            if d < best_d:
                best, best_d = j, d
    if best is None:
        return None
    cfg, sp = vals[best]
    cfg, order = cfg & 255, cfg & ~255      # (bits 8..15: the tile order's column-group width, kept)
    if cfg in (4, 8, 10) and tok == 1:
        kk = int(key.split("|")[3])
        if cfg == 4 and want % 256:
            cfg = 3           # the persistent streaming configuration covers full 256-row tiles only
        if cfg in (8, 10) and (kk % 64 or kk < 192):
            cfg = 3           # the hand-scheduled configurations need whole 64-deep K-tiles
    cfg |= order
    if tok == 3 and sp > 1:
        sp = max(1, min(sp, round(sp * want / toks[best])))
    if tok == 3 and cfg == 11:
        # the hand-scheduled weight-gradient kernel needs whole 64-token K-tiles, >= 2 in every split, the last one included:
        # fewer splits until the dispatcher's split arithmetic allows that, the 8-wave kernel when no split count does
        if want % 64 == 0:
            while sp > 1 and not cfg11_splits_ok(want // 64, sp):
                sp -= 1
        if want % 64 or not cfg11_splits_ok(want // 64, sp):
            cfg = 2
    return (cfg, sp)


def cfg11_splits_ok(nkt: int, split_k: int) -> bool:
    """The split arithmetic of the GEMM dispatcher (csrc/gemm_bf16.hip) and the test of configuration 11's launcher
    (csrc/gemm_bf16_cfg11.hip, cclip_gemm_launch_cfg11): with nkt 64-deep K-tiles and split_k requested splits, every split -
    the last, shorter one included - must hold at least two K-tiles, or the launch is refused."""
    splits = min(max(split_k, 1), nkt)
    if splits < 1:
        return False
    ktps = -(-nkt // splits)
    splits = -(-nkt // ktps)
    return ktps >= 2 and nkt - (splits - 1) * ktps >= 2


def load_tuned_table(path=None, force: bool = False) -> int:
    """Load the persisted (key -> (tile_config, split_k)) table; returns the number of entries taken."""
    import json, os
    if _TUNE_STATE["loaded"] and not force and path is None:
        return 0
    _TUNE_STATE["loaded"] = True
    env, default = _tune_paths()
    n = 0
    for cand in ([path] if path else [default, env]):       # the env file is read last: its entries win
        if cand and os.path.isfile(cand):
            try:
                with open(cand) as f:
                    blob = json.load(f)
            except (OSError, ValueError):
                continue
            if blob.get("kernel_source_hash") != kernel_source_hash():
                continue                                    # made for other kernels: tune again
            for k, v in blob.get("table", {}).items():
                _TUNED[k] = (int(v[0]), int(v[1]))
                n += 1
            _TUNE_STATE["path"] = cand
    return n


def save_tuned_table(path=None) -> str:
    import json, os
    env, default = _tune_paths()
    path = path or env or default
    blob = {"kernel_source_hash": kernel_source_hash(),
            "note": "GEMM tile configuration per (dtype, M, N, K, layout, epilogue, split) key; written by cclip_hip.ops",
            "table": {k: list(v) for k, v in sorted(_TUNED.items())}}
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "w") as f:
        json.dump(blob, f, indent=0, sort_keys=True)
    os.replace(tmp, path)
    return path


def sync_tuned_table(group=None, src: int = 0) -> None:
    """Data parallelism: every rank adopts rank `src`'s table (call once after init_process_group)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    load_tuned_table()
    box = [dict(_TUNED) if dist.get_rank(group) == src else None]
    dist.broadcast_object_list(box, src=src, group=group)
    _TUNED.clear()
    _TUNED.update(box[0])


def _collectives_live() -> bool:
    import torch.distributed as dist
    return bool(dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)


def _agree_on_choice(choice):
    """a key tuned mid-run under DP: rank 0's measurement decides for every rank (same call sequence on all ranks)"""
    import os
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1 or os.environ.get("CCLIP_TUNE_DP_SYNC", "1") == "0":
        return choice
    box = [choice]
    dist.broadcast_object_list(box, src=0)
    return tuple(box[0])


def _launch_gemm(d) -> None:
    check(d._fn(ctypes.byref(d), _stream()), "cclip_gemm_bf16")


def _time_desc(d, reps: int = 3) -> float:
    """best of three timed groups after two warm-up launches: one noisy sample must not pin a slow configuration for the run"""
    _launch_gemm(d)
    _launch_gemm(d)
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            _launch_gemm(d)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def _autotune(d, key, outs, candidates):
    """candidates: list of (tile_config, split_k).  Outputs are redirected to scratch so that in-place residual
    GEMMs (x += ...) are not applied more than once."""
    saved = (d.out_f32, d.out_bf16, d.out_pre_bf16, d.tile_config, d.split_k, d.split_ws)
    saved_cs = (d.colsum_out, d.colsum_accumulate)
    # the trials must have the GPU to themselves: with two tower streams the other tower's kernels are still running when
    # this one meets a new shape, and a candidate timed next to them can lose to a slower one timed alone
    if not torch.cuda.is_current_stream_capturing():
        torch.cuda.synchronize()
    cs_tmp = None
    if d.colsum_out:                        # trial launches must not touch (or accumulate into) the real bias gradient
        cs_tmp = torch.empty(max(d.M, d.N), device="cuda", dtype=torch.float32)
        d.colsum_out, d.colsum_accumulate = cs_tmp.data_ptr(), 0
    # scratch outputs with the SAME row stride as the real ones (outputs are often column slices of a wider slab)
    tmp = [torch.empty((d.M, d.ldc), device=t.device, dtype=t.dtype) if t is not None else None for t in outs]
    d.out_f32 = 0 if tmp[0] is None else tmp[0].data_ptr()
    d.out_bf16 = 0 if tmp[1] is None else tmp[1].data_ptr()
    d.out_pre_bf16 = 0 if tmp[2] is None else tmp[2].data_ptr()
    best, best_t = candidates[0], float("inf")
    ws = None
    for cfg, sp in candidates:
        d.tile_config, d.split_k = cfg, sp
        if sp > 1:
            need = sp * (d.M * d.N + max(d.M, d.N))
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, device=outs[0].device if outs[0] is not None else "cuda", dtype=torch.float32)
            d.split_ws = ws.data_ptr()
        try:
            t = _time_desc(d)
        except Exception:          # a configuration that does not cover this shape / epilogue (status 1: nothing launched)
            continue
        if t < best_t:
            best, best_t = (cfg, sp), t
    d.out_f32, d.out_bf16, d.out_pre_bf16, d.tile_config, d.split_k, d.split_ws = saved
    d.colsum_out, d.colsum_accumulate = saved_cs
    best = _agree_on_choice(best)
    _TUNED[key] = best
    _TUNE_STATE["misses"] += 1
    import os
    if os.environ.get("CCLIP_TUNE_FILE") or os.environ.get("CCLIP_TUNE_SAVE") == "1":
        try:
            save_tuned_table()
        except OSError:
            pass
    return best


def gemm_bf16(A: torch.Tensor, B: torch.Tensor, *, a_kcontig: bool = True, b_kcontig: bool = True,
              alpha: float = 1.0, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
              aux: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
              out_f32: Optional[torch.Tensor] = None, out_bf16: Optional[torch.Tensor] = None,
              out_pre: Optional[torch.Tensor] = None, split_k: int = 1,
              split_ws: Optional[torch.Tensor] = None, M: Optional[int] = None, tile_config: int = 0,
              split_candidates=None, scratch=None, colsum_out: Optional[torch.Tensor] = None,
              colsum_accumulate: bool = False, colsum_of_b: bool = False, ln_stats: Optional[torch.Tensor] = None,
              ln_c1: Optional[torch.Tensor] = None, rowstats_out: Optional[torch.Tensor] = None) -> None:
    """C[m][n] = epi(alpha * sum_k A(m,k) B(n,k)); see cclip_gemm_bf16 in include/cclip_hip.h.
    A: [M,K] (a_kcontig) or [K,M]; B: [N,K] (b_kcontig) or [K,N]; 2-D, inner stride 1.
    split_candidates (wgrad): list of (tile_config, split_k) to autotune over; `scratch(n)` returns an fp32
    workspace of n floats for the chosen split.
    colsum_out (wgrad layout only): fp32 [M] (+)= sum_k A(m,k), or with colsum_of_b fp32 [N] (+)= sum_k B(n,k) - the bias
    gradient, fused into the weight-gradient GEMM.
    ln_stats [M, 2] + ln_c1 [N]: LayerNorm folded into this projection; rowstats_out [N/64, M, 2]: the residual form also emits
    the 16-bit copy (out_bf16) and row statistics for the next folded projection (include/cclip_hip.h; tile configuration 8)."""
    _req16(A, "A"); _req16(B, "B")
    assert A.dim() == 2 and B.dim() == 2 and A.stride(1) == 1 and B.stride(1) == 1
    Mx, K = (A.shape[0], A.shape[1]) if a_kcontig else (A.shape[1], A.shape[0])
    N, Kb = (B.shape[0], B.shape[1]) if b_kcontig else (B.shape[1], B.shape[0])
    if M is None:
        M = Mx
    assert K == Kb, (A.shape, B.shape, a_kcontig, b_kcontig)
    outs3 = (out_f32, out_bf16, out_pre)
    outs = [t for t in outs3 if t is not None]
    assert outs, "no output"
    ldc = outs[0].stride(0)
    for t in outs:
        assert t.stride(0) == ldc and t.stride(1) == 1 and t.shape[0] >= M and t.shape[1] == N
    d = GemmDesc()
    d._fn = _fn("cclip_gemm_bf16", A, B, aux, out_bf16, out_pre)
    d.A, d.B = A.data_ptr(), B.data_ptr()
    d.a_kcontig, d.b_kcontig = int(a_kcontig), int(b_kcontig)
    d.lda, d.ldb = A.stride(0), B.stride(0)
    d.M, d.N, d.K = M, N, K
    d.alpha = alpha
    d.bias = 0 if bias is None else bias.data_ptr()
    d.act = act
    d.aux = 0 if aux is None else aux.data_ptr()
    d.ldaux = 0 if aux is None else aux.stride(0)
    d.residual = 0 if residual is None else residual.data_ptr()
    d.ldr = 0 if residual is None else residual.stride(0)
    d.out_f32 = 0 if out_f32 is None else out_f32.data_ptr()
    d.out_bf16 = 0 if out_bf16 is None else out_bf16.data_ptr()
    d.out_pre_bf16 = 0 if out_pre is None else out_pre.data_ptr()
    d.ldc = ldc
    d.split_k = split_k
    d.split_ws = 0 if split_ws is None else split_ws.data_ptr()
    d.tile_config = tile_config
    if colsum_out is not None:
        _req(colsum_out, torch.float32, "colsum_out")
        assert not a_kcontig and not b_kcontig and colsum_out.numel() == (N if colsum_of_b else M) and colsum_out.is_contiguous()
        d.colsum_out, d.colsum_accumulate, d.colsum_of_b = colsum_out.data_ptr(), int(colsum_accumulate), int(colsum_of_b)
    if ln_stats is not None or rowstats_out is not None:
        for t_, n_ in ((ln_stats, "ln_stats"), (ln_c1, "ln_c1"), (rowstats_out, "rowstats_out")):
            if t_ is not None:
                _req(t_, torch.float32, n_)
                assert t_.is_contiguous()
        d.ln_stats = 0 if ln_stats is None else ln_stats.data_ptr()
        d.ln_c1 = 0 if ln_c1 is None else ln_c1.data_ptr()
        d.rowstats_out = 0 if rowstats_out is None else rowstats_out.data_ptr()
        d.tile_config = tile_config = 8           # the only configuration with these epilogue forms
    if bias is not None:
        _req(bias, torch.float32, "bias")
    if residual is not None:
        _req(residual, torch.float32, "residual")
    if out_f32 is not None:
        _req(out_f32, torch.float32, "out_f32")
    if tile_config == 0 and AUTOTUNE and 2.0 * M * N * K >= _TUNE_MIN_FLOPS and (outs[0].is_contiguous() or True):
        if not _TUNE_STATE["loaded"]:
            load_tuned_table()
        key = _key_str((str(A.dtype).replace("torch.", ""), M, N, K, a_kcontig, b_kcontig, act, out_f32 is not None,
                        out_bf16 is not None, out_pre is not None, residual is not None, bias is not None,
                        split_k if split_candidates is None else -1, colsum_out is not None, colsum_of_b))
        choice = _TUNED.get(key)
        if choice is None:
            choice = _DERIVED.get(key)
        if choice is None:
            dp = _collectives_live()
            choice = _nearest_tuned(key, unbounded=dp)
            if choice is None and dp:
                # data parallelism: a shape only THIS rank meets (its packed row count) must not be timed here - the trial
                # launches would put a broadcast into one rank's call sequence only.  Deterministic fallback instead.
                choice = (3 if (a_kcontig and b_kcontig) else 1, split_k if split_candidates is None else split_candidates[0][1])
            if choice is not None:
                _DERIVED.put(key, choice)                      # bounded cache; never persisted, never searched
                _TUNE_STATE["derived"] = _TUNE_STATE.get("derived", 0) + 1
        if choice is None:
            cands = split_candidates if split_candidates is not None else [(c, split_k) for c in (1, 2, 3, 4, 5, 7, 8)]
            if split_candidates is None and a_kcontig and b_kcontig and split_k == 1:
                # the 256-wide configurations again with the column tiles taken in groups of g (tile_config bits 8..15): which
                # weight panels one XCD's L2 holds together - decided by timing, like the tile itself
                cands += [(c + 256 * g, split_k) for c in (3, 8) for g in (3, 4, 6) if (N + 255) // 256 > g]
            if split_candidates is None and split_k > 1:
                d.split_ws = split_ws.data_ptr()
            choice = _autotune(d, key, outs3, cands)
        if _CFG_REMAP:                                         # measurement aid (CCLIP_GEMM_REMAP="8:3,10:3"): A/B a table entry against another configuration
            choice = (_CFG_REMAP.get(choice[0], choice[0]), choice[1])
        d.tile_config, d.split_k = choice
        if d.split_k > 1 and split_candidates is not None:
            ws = scratch(d.split_k * (M * N + max(M, N)))
            d.split_ws = ws.data_ptr()
    if d.split_k > 1:
        assert d.split_ws, "split_k > 1 needs a workspace"
    if GEMM_EVENTS is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _launch_gemm(d)
        e1.record()
        GEMM_EVENTS.append((e0, e1, 2.0 * M * N * K, (int(a_kcontig), int(b_kcontig)), (M, N, K)))
        return
    _launch_gemm(d)


def rowstats_combine(partials: torch.Tensor, stats: torch.Tensor, *, rows: int, D: int, eps: float = 1e-5) -> None:
    """stats[m] = (mean, rstd) from the [nblk, rows, 2] (sum, sum of squares) partials a residual GEMM emitted (rowstats_out)"""
    _req(partials, torch.float32, "partials"); _req(stats, torch.float32, "stats")
    check(lib.cclip_rowstats_combine(_p(partials), c_int(partials.shape[0]), c_int(rows), c_int(D), c_float(eps), _p(stats), _stream()),
          "cclip_rowstats_combine")


# --------------------------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------------------------
def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, rows: int, row_index=None,
                  out_bf16=None, out_f32=None, mean=None, rstd=None, eps: float = 1e-5) -> None:
    _req(x, torch.float32, "x")
    D = x.shape[-1]
    out = out_bf16 if out_bf16 is not None else out_f32
    check(_fn("cclip_layernorm_fwd", out_bf16)(_p(x), c_long(x.stride(-2)), _p(row_index), c_int(rows), c_int(D), _p(gamma), _p(beta),
                                  c_float(eps), _p(out_bf16), _p(out_f32), c_long(out.stride(-2)), _p(mean), _p(rstd),
                                  _stream()), "cclip_layernorm_fwd")


def layernorm_bwd_ws_floats(rows: int, D: int) -> int:
    return lib.cclip_layernorm_bwd_ws_floats(c_int(rows), c_int(D))


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, *,
                  rows: int, row_index=None, dx_res=None, dx_out=None, dx_out_bf16=None, dgamma=None, dbeta=None,
                  accumulate: bool = False, ws=None) -> None:
    D = x.shape[-1]
    dxo = dx_out if dx_out is not None else dx_out_bf16
    lddx = dxo.stride(-2) if dxo is not None else x.stride(-2)
    if dx_res is not None:
        assert dx_res.stride(-2) == lddx
    if dx_out is not None and dx_out_bf16 is not None:
        assert dx_out.stride(-2) == dx_out_bf16.stride(-2)
    check(_fn("cclip_layernorm_bwd", dy, dx_out_bf16)(_p(dy), c_int(_is16(dy)), c_long(dy.stride(-2)), _p(x),
                                  c_long(x.stride(-2)), _p(row_index), c_int(rows), c_int(D), _p(gamma), _p(mean),
                                  _p(rstd), _p(dx_res), _p(dx_out), _p(dx_out_bf16), c_long(lddx), _p(dgamma),
                                  _p(dbeta), c_int(int(accumulate)), _p(ws), _stream()), "cclip_layernorm_bwd")


# --------------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------------
class AttnDesc(ctypes.Structure):
    _fields_ = [
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p),
        ("ldq", c_long), ("ldk", c_long), ("ldv", c_long),
        ("o", c_void_p), ("ldo", c_long),
        ("lse", c_void_p), ("key_keep", c_void_p),
        ("B", c_int), ("T", c_int), ("H", c_int), ("head_dim", c_int), ("causal", c_int),
        ("scale", c_float),
        ("dout", c_void_p), ("lddo", c_long),
        ("dq", c_void_p), ("dk", c_void_p), ("dv", c_void_p),
        ("lddq", c_long), ("lddk", c_long), ("lddv", c_long),
        ("o_fp8", c_void_p), ("ldo_fp8", c_long), ("o_block_scale", c_void_p), ("ld_o_block_scale", c_long),
        ("cu_seqlens", c_void_p),
    ]


def _attn_desc(q, k, v, o, lse, B, T, H, causal, key_keep, scale, head_dim=64):
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
        _req16(t, n)
        assert t.stride(-1) == 1
    d = AttnDesc()
    d.q, d.k, d.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    d.ldq, d.ldk, d.ldv = q.stride(-2), k.stride(-2), v.stride(-2)
    d.o, d.ldo = o.data_ptr(), o.stride(-2)
    d.lse = 0 if lse is None else lse.data_ptr()
    d.key_keep = 0 if key_keep is None else key_keep.data_ptr()
    d.B, d.T, d.H, d.head_dim, d.causal = B, T, H, head_dim, int(causal)
    d.scale = head_dim ** -0.5 if scale is None else scale
    return d


def _attn_cu(d, cu, B):
    if cu is not None:
        assert cu.dtype == torch.int32 and cu.is_cuda and cu.is_contiguous() and cu.numel() == B + 1
        d.cu_seqlens = cu.data_ptr()


def _attn_grads(d, dout, dq, dk, dv):
    d.dout, d.lddo = dout.data_ptr(), dout.stride(-2)
    d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    d.lddq, d.lddk, d.lddv = dq.stride(-2), dk.stride(-2), dv.stride(-2)


def _relevance_desc(q, k, v, lse, da, B, T, H, causal, scale, cu):
    """the descriptor both relevance kernels read: da (the gradient at the attention output) travels in the dout fields"""
    _req16(da, "da")
    assert da.stride(-1) == 1
    _req(lse, torch.float32, "lse")
    assert lse.is_contiguous() and lse.numel() >= B * H * T
    d = _attn_desc(q, k, v, da, lse, B, T, H, causal, None, scale)     # (o is not read: da stands in as the dtype witness)
    _attn_cu(d, cu, B)
    d.dout, d.lddo = da.data_ptr(), da.stride(-2)
    return d


def attention_fwd(q, k, v, o, *, B: int, T: int, H: int, causal: bool = False, key_keep=None, lse=None, scale=None, out_mx=None,
                  cu=None) -> None:
    """q/k/v/o: bf16 2-D views [B*T, >= H*64] (any row stride, inner stride 1); head h at columns h*64..
    out_mx = (o8 [B*T, H*64] uint8, block_scale [H*64/128, B*T, 4] uint8): the output as e4m3 + E8M0 block scales (the out-proj's
    block-scaled fp8 operand, see gemm_fp8) instead of 16-bit; `o` is then only the dtype witness and is not written.
    cu (int32 [B+1], T <= 128): packed batch - sequence b is rows [cu[b], cu[b+1]), T = the longest length."""
    d = _attn_desc(q, k, v, o, lse, B, T, H, causal, key_keep, scale)
    _attn_cu(d, cu, B)
    if out_mx is not None:
        o8, omx = out_mx
        R = o.shape[0] if cu is not None else B * T            # packed batch: the caller's row count
        assert o8.dtype == torch.uint8 and o8.stride(1) == 1 and o8.shape[0] >= R and o8.shape[1] >= H * 64 and H % 2 == 0
        _req_mx(omx, R, H * 64, "out_mx[1]")
        d.o_fp8, d.ldo_fp8, d.o_block_scale, d.ld_o_block_scale = o8.data_ptr(), o8.stride(0), omx.data_ptr(), omx.stride(0)
    check(_fn("cclip_attention_fwd", q, k, v, o)(ctypes.byref(d), _stream()), "cclip_attention_fwd")


def attention_bwd(q, k, v, o, lse, dout, dq, dk, dv, *, B: int, T: int, H: int, causal: bool = False, key_keep=None,
                  scale=None, cu=None) -> None:
    d = _attn_desc(q, k, v, o, lse, B, T, H, causal, key_keep, scale)
    _attn_cu(d, cu, B)
    _attn_grads(d, dout, dq, dk, dv)
    check(_fn("cclip_attention_bwd", q, k, v, o, dout, dq, dk, dv)(ctypes.byref(d), _stream()), "cclip_attention_bwd")


def attention_relevance(q, k, v, lse, da, R, *, B: int, T: int, H: int, causal: bool = False, scale=None, cu=None,
                        grad_scale: float = 1.0) -> None:
    """One layer's attention relevance (Chefer et al.), T <= 128: C = 1/(H grad_scale) sum_h max(P_h * dP_h, 0) with
    P = softmax(scale q k^T) (rebuilt from the forward's lse) and dP = da v^T, then R[b, :T_b, :T_b] += R[b, :T_b, :T_b] C.
    q/k/v/da as for attention_bwd (da = the gradient at the attention output); lse fp32 [B, H, T]; R fp32 [B, T, T] contiguous,
    updated in place (rows / columns >= T_b of a packed sequence are left as they are)."""
    d = _relevance_desc(q, k, v, lse, da, B, T, H, causal, scale, cu)
    _req(R, torch.float32, "R")
    assert R.is_contiguous() and tuple(R.shape) == (B, T, T), f"R: expected contiguous [{B}, {T}, {T}], got {tuple(R.shape)}"
    check(_fn("cclip_attention_relevance", q, k, v, da)(ctypes.byref(d), c_float(grad_scale), _p(R), _stream()),
          "cclip_attention_relevance")


def attention_relevance_row(q, k, v, lse, da, r_in, r_out, *, B: int, T: int, H: int, causal: bool = False, scale=None, cu=None,
                            grad_scale: float = 1.0) -> None:
    """One row of attention_relevance's update at any T <= 8192: r_out[b, :T_b] = r_in[b, :T_b] + r_in[b, :T_b] C with the same
    C (never formed), r_out[b, T_b:] = r_in[b, T_b:].  q/k/v/lse/da as for attention_relevance; r_in, r_out fp32 [B, T]
    contiguous and different buffers (the library refuses r_in is r_out)."""
    d = _relevance_desc(q, k, v, lse, da, B, T, H, causal, scale, cu)
    for r, n in ((r_in, "r_in"), (r_out, "r_out")):
        _req(r, torch.float32, n)
        assert r.is_contiguous() and tuple(r.shape) == (B, T), f"{n}: expected contiguous [{B}, {T}], got {tuple(r.shape)}"
    check(_fn("cclip_attention_relevance_row", q, k, v, da)(ctypes.byref(d), c_float(grad_scale), _p(r_in), _p(r_out), _stream()),
          "cclip_attention_relevance_row")


ATTENTION_PROBS_MAX_T = 256


def attention_probs(q, k, P, *, B: int, T: int, H: int, causal: bool = False, scale=None, key_keep=None, lse=None,
                    q_rows=None) -> None:
    """Attention probabilities of one layer: P[b, h, i, :T] = softmax_j(scale q_t k_j + mask), t = q_rows[i] (q_rows: int32
    device tensor [n_q] of query positions shared by all sequences, values outside 0 .. T-1 are clamped; None = all T
    positions).  q / k as for attention_fwd; P fp32 [B, H, n_q, >= T] with inner stride 1 (any other strides), may be
    uninitialised: every element [.., :T] is written, masked and above-diagonal entries with exactly 0.  key_keep: fp32
    [B, T], 0 masks a key.  lse is accepted for symmetry with the other attention bindings and not read (the kernel
    normalises from the scores it holds).  T <= 256."""
    if T > ATTENTION_PROBS_MAX_T:
        raise NotImplementedError(f"attention_probs: T = {T} above the kernel's limit of {ATTENTION_PROBS_MAX_T} key positions")
    for t, n in ((q, "q"), (k, "k")):
        _req16(t, n)
        assert t.dim() == 2 and t.stride(-1) == 1 and t.shape[0] >= B * T and t.shape[1] >= H * 64, \
            f"{n}: expected [>= {B * T}, >= {H * 64}] rows of heads, got {tuple(t.shape)}"
    _req(P, torch.float32, "P")
    n_q = T
    if q_rows is not None:
        assert q_rows.dtype == torch.int32 and q_rows.is_cuda and q_rows.is_contiguous() and q_rows.dim() == 1 and q_rows.numel() >= 1
        n_q = q_rows.numel()
    assert P.dim() == 4 and tuple(P.shape[:3]) == (B, H, n_q) and P.shape[3] >= T and P.stride(3) == 1, \
        f"P: expected [{B}, {H}, {n_q}, >= {T}] with inner stride 1, got {tuple(P.shape)} / {P.stride()}"
    if key_keep is not None:
        _req(key_keep, torch.float32, "key_keep")
        assert key_keep.is_contiguous() and key_keep.numel() == B * T
    d = AttnDesc()
    d.q, d.k, d.ldq, d.ldk = q.data_ptr(), k.data_ptr(), q.stride(-2), k.stride(-2)
    d.key_keep = 0 if key_keep is None else key_keep.data_ptr()
    d.B, d.T, d.H, d.head_dim, d.causal = B, T, H, 64, int(causal)
    d.scale = 64 ** -0.5 if scale is None else scale
    check(_fn("cclip_attention_probs", q, k)(ctypes.byref(d), _p(q_rows), c_int(n_q), _p(P), c_long(P.stride(0)),
                                             c_long(P.stride(1)), c_long(P.stride(2)), _stream()), "cclip_attention_probs")


# --------------------------------------------------------------------------------------------
# embedding analysis (retrieval, range search, lm_head scoring, cache classifier, k-means, coreset, spanning tree, linear probe,
# t-SNE, label spreading, concept codes, class moments, Gaussian scores): one operand contract.  Every wrapper checks in the order cuda, dtype, shape over all
# its tensors, then the size limits, then alignment, and touches the library only after that.
# --------------------------------------------------------------------------------------------
def _fits(shape, got) -> bool:
    """got against a shape in which None stands for any extent"""
    if len(got) != len(shape):
        return False
    for s, g in zip(shape, got):
        if s is not None and s != g:
            return False
    return True


def _dev_tensors(fname: str, dev, specs, *, contiguous: bool = True, host_error=TypeError, dtype_error=TypeError, device_error=ValueError):
    """The one check of a tensor argument, over specs = (t, name, dtype, shape, optional) in turn: on the device; of `dtype` (one,
    a tuple to choose from, None: any); on `dev` where one is given; of `shape` (a tuple, None in it: any extent; an int: that
    many dimensions; None: any) and contiguous unless told otherwise.  A host tensor or a non-tensor is a host_error, a wrong
    dtype a dtype_error, another device a device_error, everything else a ValueError."""
    for t, n, dtype, shape, optional in specs:
        if t is None and optional:
            continue
        if isinstance(t, torch.Tensor) and (t.is_cuda if dev is None else t.device == dev) and \
                (dtype is None or t.dtype == dtype or (dtype.__class__ is tuple and t.dtype in dtype)) and \
                (shape is None or t.shape == shape or (t.dim() == shape if shape.__class__ is int else _fits(shape, t.shape))) and \
                (not contiguous or t.is_contiguous()):
            continue                                         # all is well; below, what is not, in the contract's order
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise host_error(f"{fname}: {n}: expected a cuda tensor, got {getattr(t, 'device', type(t))} (no CPU path)")
        if dtype is not None and t.dtype != dtype and not (dtype.__class__ is tuple and t.dtype in dtype):
            names = " or ".join(str(d)[6:] for d in (dtype if isinstance(dtype, tuple) else (dtype,)))
            raise dtype_error(f"{fname}: {n}: expected {names}, got {t.dtype} on {t.device}")
        if dev is not None and t.device != dev:
            raise device_error(f"{fname}: {n} must be on {dev}, got {t.device}")
        want = ("contiguous " if contiguous else "") + (f"{shape}-D " if shape.__class__ is int else f"{list(shape)} " if shape is not None else "")
        raise ValueError(f"{fname}: {n} must be a {want}tensor (None: any extent), got {tuple(t.shape)} / {t.stride()}")


def _dev_tensor(fname: str, t, n: str, dtype, shape, dev, *, optional: bool = False, **how):
    """_dev_tensors for one tensor, which it returns"""
    _dev_tensors(fname, dev, ((t, n, dtype, shape, optional),), **how)
    return t


def _out(fname: str, t, n: str, dtype, shape, dev, *, host_error=ValueError, dtype_error=ValueError):
    """An output the caller may provide: allocated when t is None, else checked; whatever is wrong with it is a ValueError, unless
    the wrapper has always answered a host tensor or a dtype otherwise."""
    if t is None:
        return torch.empty(*shape, device=dev, dtype=dtype)
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.shape == shape and t.is_contiguous()):
        _dev_tensors(fname, dev, ((t, n, dtype, shape, False),), host_error=host_error, dtype_error=dtype_error)   # says what is wrong
    return t


def _workspace(fname: str, ws, nbytes: int, dtype, dev, *, align16: bool = False, flat: bool = False, host_error=ValueError):
    """Scratch of at least nbytes: allocated when ws is None, else the caller's contiguous `dtype` tensor (flat: a vector)."""
    size = dtype.itemsize
    if ws is None:
        return torch.empty((nbytes + size - 1) // size, device=dev, dtype=dtype)
    _dev_tensor(fname, ws, "workspace", dtype, 1 if flat else None, dev, host_error=host_error, dtype_error=host_error)
    if ws.numel() * size < nbytes or (align16 and ws.data_ptr() % 16):
        raise ValueError(f"{fname}: workspace must hold at least {nbytes} bytes{', 16-byte aligned' if align16 else ''}, got "
                         f"{ws.numel() * size} (address % 16 = {ws.data_ptr() % 16})")
    return ws


def _finite(fname: str, n: str, v, *, nonneg: bool = False) -> float:
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")) or (nonneg and v < 0):
        raise ValueError(f"{fname}: {n} must be finite{' and >= 0' if nonneg else ''}, got {v}")
    return v


_QUERIES = {}


def _query(name: str, restype, *cargs) -> int:
    """A size query of the library (the *_workspace, *_splits, *_blocks, *_parts and *_groups entries): pure functions of the sizes."""
    fn = _QUERIES.get(name)
    if fn is None:
        fn = _QUERIES[name] = getattr(lib, name)
        fn.restype = restype
    return int(fn(*cargs))


def _ld(t, *, multiple: int, at_least: int) -> int:
    """Row stride (elements) of a 2-D view.  A one-row view's is free: it is rounded down to a multiple of `multiple` and up to
    at_least, so that it fits whatever the kernel asks of a stride."""
    return t.stride(0) if t.shape[0] > 1 else max(at_least, t.stride(0) // multiple * multiple)


def _view16(fname: str, specs, dtype_error=TypeError):
    """The 16-bit row-major operands of a score kernel (csrc/score_tiles.h), first part; specs = (t, name, HALF_TYPES, None,
    False) each: all on the device, then all bfloat16 or float16, then all 2-D with inner stride 1."""
    if dtype_error is not TypeError:                         # a host tensor is a TypeError: it comes before any operand's dtype
        _dev_tensors(fname, None, [(s[0], s[1], None, None, False) for s in specs], contiguous=False)
    _dev_tensors(fname, None, specs, contiguous=False, dtype_error=dtype_error)
    for s in specs:
        if s[0].dim() != 2 or s[0].stride(1) != 1:
            raise ValueError(f"{fname}: {s[1]} must be a 2-D view with inner stride 1, got {tuple(s[0].shape)} / {s[0].stride()}")


def _limits16(fname: str, D: int, names: str, rows, *, min_d: int = 32, max_d: int = 1024):
    """Second part, once every tensor of the call has passed the first: no empty operand, D % 32 == 0 inside min_d .. max_d, row
    counts (`names`: what the messages call them) that fit the kernels' int32 indices."""
    if min(rows) >= 1 and not D % 32 and min_d <= D <= max_d and max(rows) < 2 ** 31:
        return
    shown = ", ".join(f"{k} = {v}" for k, v in zip(names.split(), rows))
    if min(rows) < 1:
        raise ValueError(f"{fname}: empty operand ({shown})")
    if D % 32 or not min_d <= D <= max_d:
        raise NotImplementedError(f"{fname}: D = {D}; the kernel needs D % 32 == 0 and {f'{min_d} <= ' if min_d else ''}D <= {max_d}")
    raise NotImplementedError(f"{fname}: {shown}; the kernel's row indices are int32 (< 2^31)")


def _ld16(fname: str, t, n: str) -> int:
    """Last part: the row stride (elements) for the kernel's 16-byte loads, a multiple of 8 from a 16-byte aligned base."""
    ld = t.stride(0) if t.shape[0] > 1 else _ld(t, multiple=8, at_least=t.shape[1])
    if ld % 8 or t.data_ptr() % 16:
        raise ValueError(f"{fname}: {n} must be 16-byte aligned with a row stride that is a multiple of 8 elements "
                         f"(stride {t.stride(0)}, address % 16 = {t.data_ptr() % 16})")
    return ld


def _pair16(fname: str, a, an: str, b, bn: str, *, dtype_error=TypeError):
    """The first part for the two operands of a score kernel, and their equal widths.  Returns (rows of a, rows of b, D).
    bfloat16 against float16 is answered where each wrapper has always answered it: by _fn, or right after this."""
    _view16(fname, ((a, an, HALF_TYPES, None, False), (b, bn, HALF_TYPES, None, False)), dtype_error)
    if b.shape[1] != a.shape[1]:
        raise ValueError(f"{fname}: {an} has {a.shape[1]} columns, {bn} has {b.shape[1]}")
    return a.shape[0], b.shape[0], a.shape[1]


SIMILARITY_TOPK_MAX_K = 64
SIMILARITY_TOPK_MAX_D = 1024


def similarity_topk_workspace(Q: int, N: int, k: int) -> int:
    """bytes of candidate workspace cclip_similarity_topk needs for this problem (Q * splits * k * 8)"""
    return _query("cclip_similarity_topk_workspace", c_long, c_int(Q), c_long(N), c_int(k))


def similarity_topk(q, g, k: int, out_scores=None, out_index=None):
    """Exact top-k of s[i, n] = <q[i], g[n]> for every query row: q [Q, D] and g [N, D] 16-bit (same dtype), inner stride 1,
    row strides multiples of 8 elements, 16-byte aligned.  Returns (scores fp32 [Q, k] descending, index int32 [Q, k]); equal
    scores by the lower gallery index, NaN last.  The Q x N matrix is never formed: the only scratch is the per-split
    candidate workspace.  1 <= k <= 64, k <= N, D % 32 == 0, D <= 1024, N < 2^31.  Enqueues two launches; no host read."""
    fname = "similarity_topk"
    Q, N, D = _pair16(fname, q, "q", g, "g")
    if not 1 <= k <= SIMILARITY_TOPK_MAX_K:
        raise ValueError(f"{fname}: k = {k} outside the kernel's range 1 .. {SIMILARITY_TOPK_MAX_K}")
    if k > N:
        raise ValueError(f"{fname}: k = {k} above the gallery's {N} rows")
    _limits16(fname, D, "Q N", (Q, N), min_d=0, max_d=SIMILARITY_TOPK_MAX_D)        # D = 0: left to the C entry, as ever
    ldq, ldg = _ld16(fname, q, "q"), _ld16(fname, g, "g")
    fn = _fn("cclip_similarity_topk", q, g)
    out_scores = _out(fname, out_scores, "out_scores", torch.float32, (Q, k), q.device, host_error=TypeError, dtype_error=TypeError)
    out_index = _out(fname, out_index, "out_index", torch.int32, (Q, k), q.device, host_error=TypeError, dtype_error=TypeError)
    nbytes = similarity_topk_workspace(Q, N, k)
    ws = _workspace(fname, None, nbytes, torch.int64, q.device)
    check(fn(_p(q), c_long(ldq), c_int(Q), _p(g), c_long(ldg), c_long(N), c_int(D), c_int(k), _p(out_scores), _p(out_index),
             _p(ws), c_long(nbytes), _stream()), "cclip_similarity_topk")
    return out_scores, out_index


def similarity_topk_biased(q, g, k: int, bias, scale: float = 1.0, out_scores=None, out_index=None):
    """Exact top-k of t[i, n] = fmaf(scale, <q[i], g[n]>, bias[n]): q, g, k and the outputs as for similarity_topk, bias a
    contiguous fp32 [N] on q's device.  Returns (t fp32 [Q, k] descending, index int32 [Q, k]); same order on t: equal t by the
    lower gallery index, NaN last.  bias[n] = -inf excludes row n (it can only trail the finite rows, by ascending index);
    scale = 1 with a zero bias is similarity_topk bit for bit.  Enqueues two launches; no host read."""
    fname = "similarity_topk_biased"
    Q, N, D = _pair16(fname, q, "q", g, "g")
    if not 1 <= k <= SIMILARITY_TOPK_MAX_K:
        raise ValueError(f"{fname}: k = {k} outside the kernel's range 1 .. {SIMILARITY_TOPK_MAX_K}")
    if k > N:
        raise ValueError(f"{fname}: k = {k} above the gallery's {N} rows")
    _limits16(fname, D, "Q N", (Q, N), min_d=0, max_d=SIMILARITY_TOPK_MAX_D)
    ldq, ldg = _ld16(fname, q, "q"), _ld16(fname, g, "g")
    fn = _fn("cclip_similarity_topk_biased", q, g)
    _dev_tensor(fname, bias, "bias", torch.float32, (N,), q.device)
    scale = float(scale)
    if scale != scale:
        raise ValueError(f"{fname}: scale is NaN")
    out_scores = _out(fname, out_scores, "out_scores", torch.float32, (Q, k), q.device, host_error=TypeError, dtype_error=TypeError)
    out_index = _out(fname, out_index, "out_index", torch.int32, (Q, k), q.device, host_error=TypeError, dtype_error=TypeError)
    nbytes = similarity_topk_workspace(Q, N, k)
    ws = _workspace(fname, None, nbytes, torch.int64, q.device)
    check(fn(_p(q), c_long(ldq), c_int(Q), _p(g), c_long(ldg), c_long(N), c_int(D), c_int(k), _p(bias), c_float(scale),
             _p(out_scores), _p(out_index), _p(ws), c_long(nbytes), _stream()), "cclip_similarity_topk_biased")
    return out_scores, out_index


def bank_lse_splits(N: int, B: int) -> int:
    """splits of the bank cclip_bank_lse works in for this problem"""
    return _query("cclip_bank_lse_splits", c_int, c_long(N), c_long(B))


def bank_lse_workspace(N: int, B: int) -> int:
    """bytes of per-split (max, sum) pairs cclip_bank_lse needs for this problem (N * splits * 8)"""
    return _query("cclip_bank_lse_workspace", c_long, c_long(N), c_long(B))


def bank_lse(g, bank, beta: float, *, out=None, workspace=None):
    """lse[j] = log sum_b exp(beta * <bank[b], g[j]>) for every gallery row: g [N, D] and bank [B, D] 16-bit (same dtype) as the
    operands of similarity_topk, each score with the bits similarity_topk returns for the pair.  Returns fp32 [N].  The B x N
    matrix is never formed; the scratch is N * splits (max, sum) pairs (`workspace`: an int64 tensor of bank_lse_workspace
    bytes, allocated when None).  B = 1 gives beta * score exactly; a NaN in gallery row j makes entry j NaN and no other; a
    non-finite bank row reaches every entry.  D % 32 == 0, D <= 1024, N, B < 2^31.  Enqueues two launches; no host read."""
    fname = "bank_lse"
    N, B, D = _pair16(fname, g, "g", bank, "bank")
    beta = _finite(fname, "beta", beta)
    _limits16(fname, D, "N B", (N, B), min_d=0, max_d=SIMILARITY_TOPK_MAX_D)
    ldg, ldb = _ld16(fname, g, "g"), _ld16(fname, bank, "bank")
    fn = _fn("cclip_bank_lse", g, bank)
    out = _out(fname, out, "out", torch.float32, (N,), g.device, host_error=TypeError, dtype_error=TypeError)
    nbytes = bank_lse_workspace(N, B)
    ws = _workspace(fname, workspace, nbytes, torch.int64, g.device)
    check(fn(_p(g), c_long(ldg), c_long(N), _p(bank), c_long(ldb), c_long(B), c_int(D), c_float(beta), _p(out), _p(ws),
             c_long(nbytes), _stream()), "cclip_bank_lse")
    return out


def similarity_range_workspace(Q: int, N: int) -> int:
    """bytes of per-(query row, gallery split) hit counts cclip_similarity_range_count fills (Q * splits * 4)"""
    return _query("cclip_similarity_range_workspace", c_long, c_int(Q), c_long(N))


def similarity_range(q, g, threshold: float, self_join: bool = False):
    """Every pair with s[i, n] = <q[i], g[n]> >= threshold, as CSR: q [Q, D] and g [N, D] as for similarity_topk (16-bit, same
    dtype, inner stride 1, row strides multiples of 8 elements, 16-byte aligned; D % 32 == 0, D <= 1024, N < 2^31).  Returns
    (offsets int64 [Q+1], index int32 [H], scores fp32 [H]): the gallery rows of query i, ascending, at offsets[i] ..
    offsets[i+1], with the score bits similarity_topk returns for the pair.  A NaN score is never a hit; threshold = -inf
    returns every other pair.  self_join (g must be q itself) keeps only the pairs n > i at about half the work.  The Q x N
    matrix is never formed.  Count launch, a cumsum over the Q * splits counts on the device, ONE host read of the total H to
    size the outputs (the only synchronisation), emit launch; H == 0 returns empty tensors and launches no emit."""
    fname = "similarity_range"
    Q, N, D = _pair16(fname, q, "q", g, "g")
    _limits16(fname, D, "Q N", (Q, N), min_d=0, max_d=SIMILARITY_TOPK_MAX_D)
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError(f"{fname}: threshold is NaN")
    ldq, ldg = _ld16(fname, q, "q"), _ld16(fname, g, "g")
    if self_join and (q.data_ptr() != g.data_ptr() or Q != N or ldq != ldg):
        raise ValueError(f"{fname}: self_join needs g to be q itself (same memory, same rows), got Q = {Q}, N = {N}")
    count = _fn("cclip_similarity_range_count", q, g)
    emit = _fn("cclip_similarity_range_emit", q, g)
    nbytes = similarity_range_workspace(Q, N)
    splits = nbytes // (4 * Q)
    counts = torch.empty(Q * splits, device=q.device, dtype=torch.int32)
    head = (_p(q), c_long(ldq), c_int(Q), _p(g), c_long(ldg), c_long(N), c_int(D), c_float(threshold), c_int(int(bool(self_join))))
    check(count(*head, _p(counts), c_long(nbytes), _stream()), "cclip_similarity_range_count")
    starts = torch.zeros(Q * splits + 1, device=q.device, dtype=torch.int64)   # exclusive scan, the total last
    torch.cumsum(counts, 0, dtype=torch.int64, out=starts[1:])
    offsets = starts[::splits].contiguous()
    H = int(starts[-1].item())                                                  # the one host read
    index = torch.empty(H, device=q.device, dtype=torch.int32)
    scores = torch.empty(H, device=q.device, dtype=torch.float32)
    if H > 0:
        check(emit(*head, _p(starts), c_long(H), c_long(H), _p(index), _p(scores), _stream()), "cclip_similarity_range_emit")
    return offsets, index, scores


LM_HEAD_SCORE_MAX_D = 1024


def lm_head_score_workspace(R: int, V: int) -> int:
    """bytes of per-split partials cclip_lm_head_score needs (R * ceil(V / 1024) * 24)"""
    return _query("cclip_lm_head_score_workspace", c_long, c_int(R), c_int(V))


def lm_head_score(x16, w16, labels_i32, *, ignore_index: int = -100, logp=None, lse=None, pred=None, pred_logit=None):
    """Scores of the lm_head rows z = x16 @ w16^T without the logits: x16 [R, D] and w16 [V, D] 16-bit (same dtype), inner
    stride 1, row strides multiples of 8 elements, 16-byte aligned; labels_i32 int32 [R].  Returns (logp, lse, pred,
    pred_logit), each [R]: logp = z[label] - lse (exactly 0 where label == ignore_index, NaN for any other label outside
    [0, V)), lse = logsumexp(z), pred = argmax (equal logits: the lower column; NaN below every number) and its logit.
    D % 32 == 0, 32 <= D <= 1024.  A row's outputs do not depend on R.  Enqueues two launches; no host read."""
    fname = "lm_head_score"
    # this wrapper answers a wrong dtype, mixed dtypes and V >= 2^31 with a ValueError (the others: TypeError, NotImplementedError)
    R, V, D = _pair16(fname, x16, "x16", w16, "w16", dtype_error=ValueError)
    if w16.dtype != x16.dtype:
        raise ValueError(f"{fname}: x16 and w16 must be bfloat16 or float16, both alike, got {x16.dtype} / {w16.dtype}")
    dev = x16.device
    _dev_tensor(fname, labels_i32, "labels_i32", torch.int32, (R,), None, dtype_error=ValueError)
    if V >= 2 ** 31:
        raise ValueError(f"{fname}: V = {V}; column indices are int32")
    _limits16(fname, D, "R V", (R, V), max_d=LM_HEAD_SCORE_MAX_D)
    ldx, ldw = _ld16(fname, x16, "x16"), _ld16(fname, w16, "w16")
    fn = _fn("cclip_lm_head_score", x16, w16)
    outs = tuple(_out(fname, t, n, dt, (R,), dev) for t, n, dt in ((logp, "logp", torch.float32), (lse, "lse", torch.float32),
                                                                   (pred, "pred", torch.int32), (pred_logit, "pred_logit", torch.float32)))
    ws = _workspace(fname, None, lm_head_score_workspace(R, V), torch.int64, dev)
    check(fn(_p(x16), c_long(ldx), c_int(R), c_int(D), _p(w16), c_long(ldw), c_int(V), _p(labels_i32), c_int(ignore_index),
             _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(ws), _stream()), "cclip_lm_head_score")
    return outs


CACHE_AFFINITY_MAX_C = 256
CACHE_AFFINITY_MAX_D = 1024


def cache_layout(labels, num_classes: int):
    """The class-grouped layout cclip_cache_affinity reads: labels (N integers in [0, num_classes), a tensor or a sequence) ->
    (gather int64 [Np], class_off int32 [num_classes + 1], class_len int32 [num_classes]), all on the host.  Class c owns the
    laid-out rows class_off[c] .. class_off[c + 1], a segment of ceil(class_len[c] / 16) * 16 rows (none for an empty class);
    gather[j] is the original row that laid-out row j holds, -1 for padding.  A stable sort by class: the rows of a class keep
    their original order.  Pure host code, needs no library."""
    num_classes = int(num_classes)
    if num_classes < 1:
        raise ValueError(f"cache_layout: num_classes = {num_classes}")
    lab = torch.as_tensor(labels).detach().cpu()
    if lab.dim() != 1 or ((lab.is_floating_point() or lab.dtype == torch.bool) and lab.numel()):
        raise ValueError(f"cache_layout: labels must be a 1-D integer vector, got {tuple(lab.shape)} {lab.dtype}")
    lab = lab.long()
    if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= num_classes):
        raise ValueError(f"cache_layout: labels outside [0, {num_classes}): min {int(lab.min())}, max {int(lab.max())}")
    count = torch.bincount(lab, minlength=num_classes)
    seg = (count + 15) // 16 * 16
    off = torch.zeros(num_classes + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(seg, 0)
    if int(off[-1]) >= 2 ** 31:
        raise ValueError(f"cache_layout: {int(off[-1])} laid-out rows; the kernel's row index is int32")
    order = torch.sort(lab, stable=True).indices
    start = torch.cumsum(count, 0) - count                      # first sorted position of each class
    sl = lab[order]
    gather = torch.full((int(off[-1]),), -1, dtype=torch.int64)
    gather[off[:-1][sl] + torch.arange(lab.numel()) - start[sl]] = order
    return gather, off.to(torch.int32), count.to(torch.int32)


def _check_cache_segments(class_off, class_len, Np: int):
    """The content contract of the two layout arrays (include/cclip_hip.h), checked here because the C entry only sees
    device pointers.  Returns C."""
    for t, n in ((class_off, "class_off"), (class_len, "class_len")):
        if not isinstance(t, torch.Tensor) or t.is_cuda or t.dtype != torch.int32:
            raise TypeError(f"cache_affinity: {n}: expected a host int32 tensor (cache_layout's), got "
                            f"{getattr(t, 'device', type(t))} {getattr(t, 'dtype', '')}")
        if t.dim() != 1:
            raise ValueError(f"cache_affinity: {n} must be 1-D, got {tuple(t.shape)}")
    C = class_len.numel()
    if class_off.numel() != C + 1:
        raise ValueError(f"cache_affinity: class_off has {class_off.numel()} entries for {C} classes (expected C + 1)")
    if not 1 <= C <= CACHE_AFFINITY_MAX_C:
        raise NotImplementedError(f"cache_affinity: C = {C}; the kernel takes 1 .. {CACHE_AFFINITY_MAX_C} classes")
    off, ln = class_off.long(), class_len.long()
    width = off[1:] - off[:-1]
    if int(off[0]) != 0 or int(off[-1]) != Np or bool((off % 16 != 0).any()) or bool((width < 0).any()):
        raise ValueError(f"cache_affinity: class_off must start at 0, ascend in multiples of 16 and end at the {Np} stored rows")
    if bool((ln < 0).any()) or bool((ln > width).any()):
        raise ValueError("cache_affinity: class_len must lie in 0 .. the width of its segment")
    return C


_CACHE_SEGMENTS = {}       # (device, class_off bytes, class_len bytes) -> the two device copies (bounded; oldest evicted first)


def _cache_segments_on(dev, class_off, class_len):
    key = (str(dev), class_off.numpy().tobytes(), class_len.numpy().tobytes())
    hit = _CACHE_SEGMENTS.get(key)
    if hit is None:
        if len(_CACHE_SEGMENTS) >= 16:
            _CACHE_SEGMENTS.pop(next(iter(_CACHE_SEGMENTS)))
        hit = _CACHE_SEGMENTS[key] = (class_off.contiguous().to(dev), class_len.contiguous().to(dev))
    return hit


def cache_affinity_workspace(Q: int, Np: int, C: int) -> int:
    """bytes of per-split class sums cclip_cache_affinity needs (Q * splits(Np) * C * 4; 0 for a problem it would refuse)"""
    return _query("cclip_cache_affinity_workspace", c_long, c_int(Q), c_long(Np), c_int(C))


def _cache_operands(fname: str, q, g, class_off, class_len, beta, exclude):
    """The argument checks cache_affinity and cache_affinity_backward share.  Returns (Q, Np, D, C, ldq, ldg, beta)."""
    Q, Np, D = _pair16(fname, q, "q", g, "g")
    C = _check_cache_segments(class_off, class_len, Np)
    beta = _finite(fname, "beta", beta)
    _limits16(fname, D, "Q Np", (Q, Np), max_d=CACHE_AFFINITY_MAX_D)
    ldq, ldg = _ld16(fname, q, "q"), _ld16(fname, g, "g")
    if g.dtype != q.dtype:
        raise TypeError(f"{fname}: mixed bfloat16 / float16 operands")
    if g.device != q.device:
        raise TypeError(f"{fname}: q on {q.device}, g on {g.device}")
    _dev_tensor(fname, exclude, "exclude", torch.int32, (Q,), q.device, optional=True)
    return Q, Np, D, C, ldq, ldg, beta


def cache_affinity(q, g, class_off, class_len, beta: float, *, exclude=None, out=None):
    """Class affinities A[i, c] = sum over the live rows n of class c, n != exclude[i], of exp(beta * (<q[i], g[n]> - 1)):
    q [Q, D] and g [Np, D] 16-bit (same dtype), inner stride 1, row strides multiples of 8 elements, 16-byte aligned; g laid
    out by class as cache_layout describes, padding rows allocated (their content is never used).  class_off / class_len:
    cache_layout's HOST int32 vectors - their content is checked here, on the host, and their device copies are kept per
    layout, so a call reads nothing back.  exclude: int32 [Q] on the device, a row of g per query to leave out (-1: none).
    Returns fp32 [Q, C]; an empty class is exactly 0.  The Q x Np matrix is never formed: the only scratch is the per-split
    workspace.  1 <= C <= 256, D % 32 == 0, 32 <= D <= 1024, Np < 2^31.  A query's row does not depend on Q.  Enqueues two
    launches; no host read."""
    fname = "cache_affinity"
    Q, Np, D, C, ldq, ldg, beta = _cache_operands(fname, q, g, class_off, class_len, beta, exclude)
    dev = q.device
    out = _out(fname, out, "out", torch.float32, (Q, C), dev, host_error=TypeError, dtype_error=TypeError)
    off_d, len_d = _cache_segments_on(dev, class_off, class_len)
    nbytes = cache_affinity_workspace(Q, Np, C)
    ws = _workspace(fname, None, nbytes, torch.float32, dev)
    check(_fn("cclip_cache_affinity", q, g)(_p(q), c_long(ldq), c_int(Q), _p(g), c_long(ldg), c_long(Np), c_int(D), _p(off_d), _p(len_d),
                                            c_int(C), c_float(beta), _p(exclude), _p(out), _p(ws), c_long(nbytes), _stream()),
          "cclip_cache_affinity")
    return out


def cache_affinity_backward(q, g, class_off, class_len, beta: float, dA, *, exclude=None, out=None):
    """Gradient of cache_affinity's A with respect to the stored rows: operands, layout and limits as there; dA fp32 [Q, C]
    contiguous on the device.  Returns dG fp32 [Np, D]:
        dG[n] = beta * sum over the queries i with n != exclude[i] of dA[i, c(n)] * exp(beta * (<q[i], g[n]> - 1)) * q[i]
    for the live rows and exactly +0.0 for the padding rows; every row is written (`out` needs no zero fill), a padding row's
    content (NaN) never reaches it, and the Q x Np matrix is never formed.  No atomics: two launches are bitwise equal.
    Enqueues two launches; no host read."""
    fname = "cache_affinity_backward"
    Q, Np, D, C, ldq, ldg, beta = _cache_operands(fname, q, g, class_off, class_len, beta, exclude)
    dev = q.device
    _dev_tensor(fname, dA, "dA", torch.float32, (Q, C), dev)
    out = _out(fname, out, "out", torch.float32, (Np, D), dev, host_error=TypeError, dtype_error=TypeError)
    off_d, len_d = _cache_segments_on(dev, class_off, class_len)
    nbytes = _query("cclip_cache_affinity_bwd_workspace", c_long, c_int(Q), c_int(C))
    ws = _workspace(fname, None, nbytes, torch.float32, dev)
    check(_fn("cclip_cache_affinity_bwd", q, g)(_p(q), c_long(ldq), c_int(Q), _p(g), c_long(ldg), c_long(Np), c_int(D), _p(off_d),
                                                _p(len_d), c_int(C), c_float(beta), _p(exclude), _p(dA), _p(out), _p(ws), c_long(nbytes),
                                                _stream()), "cclip_cache_affinity_bwd")
    return out


KMEANS_MAX_D = 1024


def _kmeans_operands(fname: str, x, c, cn: str):
    """The argument checks of the wrappers that take rows x and centroids (or concepts) c.  Returns (N, K, D, ldx, ldc)."""
    N, K, D = _pair16(fname, x, "x", c, cn)
    _limits16(fname, D, "N K", (N, K), max_d=KMEANS_MAX_D)
    if c.device != x.device:
        raise TypeError(f"{fname}: x on {x.device}, {cn} on {c.device}")
    if c.dtype != x.dtype:
        raise TypeError(f"{fname}: mixed bfloat16 / float16 operands")
    return N, K, D, _ld16(fname, x, "x"), _ld16(fname, c, cn)


def kmeans_assign(x, c, *, want_second: bool = False, out_assign=None, out_best=None, out_second=None):
    """The assignment step of k-means: for every row of x [N, D] the centroid of c [K, D] with the largest <x[n], c[k]>.  Both
    16-bit (same dtype), inner stride 1, row strides multiples of 8 elements, 16-byte aligned.  Returns (assign int32 [N], best
    fp32 [N], second fp32 [N] or None): the centroid, its score and - with want_second or out_second - the row's second-largest
    score (NaN if K == 1).  Equal scores go to the lower centroid, NaN ranks below every number; the three are bit for bit what
    similarity_topk(x, c, min(2, K)) returns.  The N x K matrix is never formed and there is no workspace.  D % 32 == 0,
    32 <= D <= 1024, N and K < 2^31.  A row's outputs do not depend on N.  Enqueues one launch; no host read."""
    fname = "kmeans_assign"
    N, K, D, ldx, ldc = _kmeans_operands(fname, x, c, "c")
    dev = x.device
    out_assign = _out(fname, out_assign, "out_assign", torch.int32, (N,), dev)
    out_best = _out(fname, out_best, "out_best", torch.float32, (N,), dev)
    if want_second or out_second is not None:
        out_second = _out(fname, out_second, "out_second", torch.float32, (N,), dev)
    fn = _fn("cclip_kmeans_assign", x, c)
    check(fn(_p(x), c_long(ldx), c_long(N), _p(c), c_long(ldc), c_long(K), c_int(D), _p(out_assign), _p(out_best), _p(out_second),
             _stream()), "cclip_kmeans_assign")
    return out_assign, out_best, out_second


def kmeans_update_workspace(N: int, K: int, D: int) -> int:
    """bytes of per-slab partial sums cclip_kmeans_update needs ((ceil(N / 256) + K) * D * 4; 0 for a problem it would refuse)"""
    return _query("cclip_kmeans_update_workspace", c_long, c_long(N), c_long(K), c_int(D))


def kmeans_update(x, assign, K: int, prev_c, *, out_c=None, out_norm=None, check_range: bool = True):
    """The centroid step of spherical k-means: x [N, D] 16-bit as for kmeans_assign, assign an int32 / int64 [N] device vector
    of cluster ids in [0, K), prev_c [K, D] of x's dtype (inner stride 1).  Returns (c16 [K, D], norm fp32 [K], counts int64
    [K]): with S = the fp32 sum of the rows of cluster k, norm[k] = |S| and c16[k] = S / |S| rounded once to the 16-bit type;
    an empty cluster, and one whose rows cancel to zero or whose sum is not finite, keeps prev_c[k] bit for bit with norm 0.
    out_c may be prev_c.  The grouping is plumbing in torch on the device: a stable sort of assign (`order`: the rows by
    cluster, ascending inside a cluster - a permutation by construction) and the boundaries seg_off[k] = the number of entries
    below k, found in the sorted ids (monotone, from 0 to N, by construction); counts are their differences, the exact
    bincount, without bincount's hidden host read.  What the construction needs is ids inside [0, K): an id outside is a
    ValueError, caught by ONE device-side min / max read back together and nothing else; check_range=False skips that read for
    an assign that comes straight from kmeans_assign against K centroids.  No float atomics: two calls are bitwise equal.
    Enqueues two launches."""
    fname = "kmeans_update"
    N, Kp, D, ldx, ldp = _kmeans_operands(fname, x, prev_c, "prev_c")
    K = int(K)
    if Kp != K:
        raise ValueError(f"{fname}: prev_c has {Kp} rows for K = {K}")
    dev = x.device
    _dev_tensor(fname, assign, "assign", (torch.int32, torch.int64), (N,), dev, contiguous=False)
    if out_c is not None:
        _dev_tensor(fname, out_c, "out_c", x.dtype, (K, D), dev, contiguous=False, host_error=ValueError, dtype_error=ValueError)
        if out_c.stride(1) != 1 or (K > 1 and out_c.stride(0) < D):
            raise ValueError(f"{fname}: out_c must have inner stride 1 and rows that do not overlap, got strides {out_c.stride()}")
    out_norm = _out(fname, out_norm, "out_norm", torch.float32, (K,), dev)
    if check_range:
        lo, hi = torch.stack([assign.min(), assign.max()]).tolist()             # the one host read
        if lo < 0 or hi >= K:
            raise ValueError(f"{fname}: assign outside [0, {K}): min {lo}, max {hi}")
    if out_c is None:
        out_c = torch.empty(K, D, device=dev, dtype=x.dtype)
    ids, order = torch.sort(assign, stable=True)
    seg_off = torch.searchsorted(ids, torch.arange(K + 1, device=dev, dtype=ids.dtype)).to(torch.int32)
    counts = seg_off.diff().long()
    order = order.to(torch.int32)
    nbytes = kmeans_update_workspace(N, K, D)
    ws = _workspace(fname, None, nbytes, torch.float32, dev)
    fn = _fn("cclip_kmeans_update", x, prev_c)
    ldo = _ld(out_c, multiple=1, at_least=D)
    check(fn(_p(x), c_long(ldx), c_long(N), c_int(D), _p(order), _p(seg_off), c_long(K), _p(prev_c), c_long(ldp), _p(out_c),
             c_long(ldo), _p(out_norm), _p(ws), c_long(nbytes), _stream()), "cclip_kmeans_update")
    return out_c, out_norm, counts


CORESET_FROM_PARTIALS, CORESET_SCAN_ONLY = -1, -2        # the `centre` modes of cclip_coreset_step (include/cclip_hip.h)


def coreset_blocks(N: int) -> int:
    """work-groups of one cclip_coreset_step launch = keys per partial buffer: min(1024, ceil(N / 64)); 0 for an N it would refuse"""
    return _query("cclip_coreset_blocks", c_int, c_long(N))


def coreset_workspace(N: int) -> int:
    """bytes of the two partial-key buffers cclip_coreset_greedy alternates between (2 * coreset_blocks(N) * 8)"""
    return _query("cclip_coreset_workspace", c_long, c_long(N))


def _rows16_state(fname: str, x, *vectors):
    """The argument checks of the wrappers over one 16-bit operand x (as for kmeans_assign) and its per-row state `vectors`,
    (t, name, dtype, optional) each: [N], contiguous on x's device.  Returns (N, D, ldx)."""
    _view16(fname, ((x, "x", HALF_TYPES, None, False),))
    N, D = x.shape
    _limits16(fname, D, "N", (N,), max_d=KMEANS_MAX_D)
    _dev_tensors(fname, x.device, [(t, n, dt, (N,), optional) for t, n, dt, optional in vectors], dtype_error=ValueError)
    return N, D, _ld16(fname, x, "x")


def coreset_step(x, mind, owner, partial_out, *, centre: Optional[int] = None, partial_in=None, scan_only: bool = False, weight=None,
                 out_pick=None, out_radius=None):
    """One k-centre greedy pick over the unit 16-bit rows x [N, D] (inner stride 1, row stride a multiple of 8 elements, 16-byte
    aligned), in place on the state mind fp32 [N] (cosine distance to the nearest centre so far, +inf = none) and owner int32 [N]
    (that centre's row, -1 = none, owner[i] == i = the row is a centre).  partial_in / partial_out: two different int64
    [coreset_blocks(N)] key buffers (a key: the order image of weight * mind above ~row; 0 = no eligible row).  The centre c is
    `centre` (an int in [0, N)), or - centre None - the row of the largest key of partial_in; scan_only=True takes no centre and
    updates nothing.  With a centre: pick = c, radius = mind[c] before the update, mind[c] = 0, owner[c] = c, and every other
    non-centre row with 1 - <x_i, x_c> strictly below mind[i] takes that distance and owner c.  partial_out then holds every
    work-group's best eligible key: owner[i] != i and weight[i] > 0 where weight fp32 [N] is given (a NaN weight is never
    eligible), larger weight * mind first, equal values to the lower row.  Returns (pick int32 [1], radius fp32 [1]) - pick -1
    and radius NaN when partial_in holds no eligible row - or (None, None) for scan_only.  D % 32 == 0, 32 <= D <= 1024,
    N < 2^31.  No atomics: two calls from equal states are bitwise equal.  Enqueues one launch; no host read."""
    fname = "coreset_step"
    N, D, ldx = _rows16_state(fname, x, (mind, "mind", torch.float32, False), (owner, "owner", torch.int32, False),
                              (weight, "weight", torch.float32, True))
    dev, P = x.device, coreset_blocks(N)
    _dev_tensors(fname, dev, ((partial_out, "partial_out", torch.int64, (P,), False), (partial_in, "partial_in", torch.int64, (P,), True)),
                 host_error=ValueError, dtype_error=ValueError)
    if scan_only:
        if centre is not None:
            raise ValueError(f"{fname}: scan_only takes no centre")
        mode = CORESET_SCAN_ONLY
    elif centre is None:
        if partial_in is None:
            raise ValueError(f"{fname}: without a centre the pick comes from partial_in")
        mode = CORESET_FROM_PARTIALS
    else:
        mode = int(centre)
        if not 0 <= mode < N:
            raise ValueError(f"{fname}: centre = {centre} outside [0, {N})")
    if partial_in is not None and partial_in.data_ptr() == partial_out.data_ptr():
        raise ValueError(f"{fname}: partial_in and partial_out must be different buffers (other work-groups still read the old keys)")
    if not scan_only:
        out_pick = _out(fname, out_pick, "out_pick", torch.int32, (1,), dev)
        out_radius = _out(fname, out_radius, "out_radius", torch.float32, (1,), dev)
    else:
        out_pick = out_radius = None
    fn = _fn("cclip_coreset_step", x)
    check(fn(_p(x), c_long(ldx), c_long(N), c_int(D), _p(weight), _p(mind), _p(owner), c_int(mode), _p(partial_in), _p(partial_out),
             _p(out_pick), _p(out_radius), _stream()), "cclip_coreset_step")
    return out_pick, out_radius


def coreset_greedy(x, mind, owner, m: int, *, first: Optional[int] = None, workspace=None, weight=None, out_picks=None,
                   out_radius=None):
    """m k-centre greedy picks (m launches of `coreset_step`, enqueued by one native call) on the state of `coreset_step`.
    workspace: int64 [2, coreset_blocks(N)], the two key buffers; pick t reads workspace[t % 2] and writes the other.  first an
    int in [0, N): pick 0 takes that row; first None: workspace[0] already holds the keys of the state (a scan_only step into
    it).  Returns (picks int32 [m], radius fp32 [m], workspace): bit for bit what m single steps give; the state's keys end in
    workspace[m % 2].  Once no eligible row is left the picks are -1 with radius NaN.  m == 0 launches nothing.  No host read."""
    fname = "coreset_greedy"
    N, D, ldx = _rows16_state(fname, x, (mind, "mind", torch.float32, False), (owner, "owner", torch.int32, False),
                              (weight, "weight", torch.float32, True))
    dev, P = x.device, coreset_blocks(N)
    m = int(m)
    if not 0 <= m <= N:
        raise ValueError(f"{fname}: m = {m} outside [0, {N}]")
    if first is None:
        if workspace is None:
            raise ValueError(f"{fname}: without a first row workspace[0] must hold the keys of the state")
        mode = CORESET_FROM_PARTIALS
    else:
        mode = int(first)
        if not 0 <= mode < N:
            raise ValueError(f"{fname}: first = {first} outside [0, {N})")
    if workspace is None:                                    # the two key buffers by shape, zeroed: not scratch sized in bytes
        workspace = torch.zeros(2, P, device=dev, dtype=torch.int64)
    _dev_tensor(fname, workspace, "workspace", torch.int64, (2, P), dev, host_error=ValueError, dtype_error=ValueError)
    out_picks = _out(fname, out_picks, "out_picks", torch.int32, (m,), dev)
    out_radius = _out(fname, out_radius, "out_radius", torch.float32, (m,), dev)
    fn = _fn("cclip_coreset_greedy", x)
    check(fn(_p(x), c_long(ldx), c_long(N), c_int(D), _p(weight), _p(mind), _p(owner), c_int(mode), c_long(m), _p(out_picks),
             _p(out_radius), _p(workspace), c_long(workspace.numel() * 8), _stream()), "cclip_coreset_greedy")
    return out_picks, out_radius, workspace


def mst_workspace(N: int) -> int:
    """bytes of scratch cclip_mst_boruvka needs (32 N + 256: the row keys, the component keys, the parents, two label buffers,
    the round flags); 0 for an N it would refuse"""
    return _query("cclip_mst_workspace", c_long, c_long(N))


def mreach_nearest_splits(N: int) -> int:
    """gallery splits of one cclip_mreach_nearest launch (a function of N alone); 0 for an N it would refuse"""
    return _query("cclip_mreach_nearest_splits", c_int, c_long(N))


def mreach_nearest(x, core, comp, *, out=None):
    """For every row i of the unit 16-bit rows x [N, D] (inner stride 1, row stride a multiple of 8 elements, 16-byte aligned)
    the closest row j outside i's component under mutual-reachability similarity m = min(<x_i, x_j>, core[i], core[j]): core
    fp32 [N], comp int32 [N] (any values: only compared).  Returns keys int64 [N]: the order image of m in the high word above
    ~j, the largest over the rows j with comp[j] != comp[i] - larger m first, equal m to the lower j, a NaN m below every
    number - or 0 where no such row exists.  The score carries the bits similarity_topk returns for the pair; the N x N matrix
    is never formed.  Integer atomics only where the gallery is split: two calls are bitwise equal.  D % 32 == 0,
    32 <= D <= 1024, N < 2^31.  No host read."""
    fname = "mreach_nearest"
    N, D, ldx = _rows16_state(fname, x, (core, "core", torch.float32, False))
    _dev_tensor(fname, comp, "comp", torch.int32, (N,), x.device, dtype_error=ValueError)
    out = _out(fname, out, "out", torch.int64, (N,), x.device)
    fn = _fn("cclip_mreach_nearest", x)
    check(fn(_p(x), c_long(ldx), c_long(N), c_int(D), _p(core), _p(comp), _p(out), _stream()), "cclip_mreach_nearest")
    return out


def mst_boruvka(x, core, *, workspace=None):
    """The maximum spanning tree of the complete graph on the rows of x under mutual-reachability similarity (x, core as for
    `mreach_nearest`), unique under the strict total order "larger m, then smaller min(i, j), then smaller max(i, j)".
    Returns (u int32 [N], v int32 [N], m fp32 [N]): N - 1 slots hold an edge with its m, exactly one holds u = v = -1 and
    m = NaN (N == 1: that slot alone).  ceil(log2 N) Boruvka rounds are enqueued by one native call; a device flag ends the
    work once one component is left.  workspace: an int64 tensor of at least mst_workspace(N) bytes.  Two calls are bitwise
    equal.  No host read."""
    fname = "mst_boruvka"
    N, D, ldx = _rows16_state(fname, x, (core, "core", torch.float32, False))
    dev = x.device
    workspace = _workspace(fname, workspace, mst_workspace(N), torch.int64, dev)
    u = torch.empty(N, device=dev, dtype=torch.int32)
    v = torch.empty(N, device=dev, dtype=torch.int32)
    m = torch.empty(N, device=dev, dtype=torch.float32)
    fn = _fn("cclip_mst_boruvka", x)
    check(fn(_p(x), c_long(ldx), c_long(N), c_int(D), _p(core), _p(u), _p(v), _p(m), _p(workspace), c_long(workspace.numel() * 8),
             _stream()), "cclip_mst_boruvka")
    return u, v, m


PROBE_MAX_C = 256
PROBE_MAX_D = 1024


def probe_workspace(N: int, C: int, D: int) -> int:
    """bytes of workspace cclip_probe_forward / cclip_probe_backward need (the hi + lo image of W, the per-slot partials of dW
    and db, the reduction tree: include/cclip_hip.h states the closed form; 0 for a problem they would refuse)"""
    return _query("cclip_probe_workspace", c_long, c_long(N), c_int(C), c_int(D))


def probe_parts(N: int, C: int, D: int) -> int:
    """the number of partial slots the backward's rows are split into: a function of (N, C, D) alone"""
    return _query("cclip_probe_parts", c_int, c_long(N), c_int(C), c_int(D))


def _probe_operands(fname: str, x, W, bias, labels, row_weight):
    """The argument checks probe_forward and probe_backward share.  Returns (N, C, D, ldx)."""
    _view16(fname, ((x, "x", HALF_TYPES, None, False),))
    (N, D), dev = x.shape, x.device
    C = _dev_tensor(fname, W, "W", torch.float32, (None, D), dev, device_error=TypeError).shape[0]   # an operand, like c and g
    _limits16(fname, D, "N", (N,), max_d=PROBE_MAX_D)
    if not 2 <= C <= PROBE_MAX_C:
        raise NotImplementedError(f"{fname}: C = {C}; the kernel takes 2 .. {PROBE_MAX_C} classes")
    _dev_tensors(fname, dev, ((bias, "bias", torch.float32, (C,), True), (labels, "labels", torch.int32, (N,), True),
                              (row_weight, "row_weight", torch.float32, (N,), True)), host_error=ValueError, dtype_error=ValueError)
    return N, C, D, _ld16(fname, x, "x")


def probe_forward(x, W, bias, labels, row_weight=None, logits: bool = False, out=None):
    """One pass of a linear probe over x [N, D] (16-bit, inner stride 1, row stride a multiple of 8 elements, 16-byte aligned)
    with W fp32 [C, D], bias fp32 [C] or None, labels int32 [N] or None (a label outside [0, C): the row is ignored) and
    row_weight fp32 [N] or None (clamped into [0, 1], NaN -> 0).  Returns (lse fp32 [N], loss fp32 [N], pred int32 [N], logits
    fp32 [N, C] or None): the logits are those of the 16-bit pair hi + lo of W (include/cclip_hip.h), loss[n] =
    row_weight[n] * (lse[n] - z[n, labels[n]]) and exactly +0.0 for an ignored or zero-weight row, pred the argmax (ties to the
    lower class, NaN lowest).  `out`: a tuple of tensors to write those into.  The N x C matrix is written only with logits=True.
    A row's outputs do not depend on N.  2 <= C <= 256, D % 32 == 0, 32 <= D <= 1024.  Enqueues two launches; no host read."""
    fname = "probe_forward"
    N, C, D, ldx = _probe_operands(fname, x, W, bias, labels, row_weight)
    dev = x.device
    o = tuple(out) if out is not None else (None, None, None, None)
    if len(o) not in (3, 4):
        raise ValueError(f"{fname}: out must be (lse, loss, pred) or (lse, loss, pred, logits)")
    lse = _out(fname, o[0], "lse", torch.float32, (N,), dev)
    loss = _out(fname, o[1], "loss", torch.float32, (N,), dev)
    pred = _out(fname, o[2], "pred", torch.int32, (N,), dev)
    z = None
    if logits or (len(o) == 4 and o[3] is not None):
        z = _out(fname, o[3] if len(o) == 4 else None, "logits", torch.float32, (N, C), dev)
    nbytes = probe_workspace(N, C, D)
    ws = _workspace(fname, None, nbytes, torch.float32, dev)
    fn = _fn("cclip_probe_forward", x)
    check(fn(_p(x), c_long(ldx), c_long(N), c_int(D), _p(W), _p(bias), c_int(C), _p(labels), _p(row_weight), _p(lse), _p(loss),
             _p(pred), _p(z), _p(ws), c_long(nbytes), _stream()), "cclip_probe_forward")
    return lse, loss, pred, z


def probe_backward(x, W, bias, labels, lse, scale: float, l2: float, row_weight=None, loss=None, out=None):
    """Gradient of the probe's objective at the operands of probe_forward, whose `lse` (and `loss`, for the scalar) it takes.
    Returns (dW fp32 [C, D], db fp32 [C], objective fp32 [1] or None):
        dW = scale * sum_n g[n, :]^T x[n, :] + l2 * W,  db = scale * sum_n g[n, :],  g[n, c] = rw[n] (softmax(z[n])[c] - [c == y_n])
        objective = scale * sum(loss) + l2 / 2 * sum(W^2)       (with `loss`)
    of the function of hi + lo the forward evaluates; ignored rows contribute exactly nothing.  `scale` is 1 / (sum of the live
    rows' weights), the caller's.  `out`: (dW, db) or (dW, db, objective) to write into.  The rows are split over the grid and
    the partial sums merged in a fixed order: no atomics, two calls are bitwise equal.  Enqueues three launches, four with the
    objective; no host read."""
    fname = "probe_backward"
    N, C, D, ldx = _probe_operands(fname, x, W, bias, labels, row_weight)
    dev = x.device
    scale, l2 = _finite(fname, "scale", scale, nonneg=True), _finite(fname, "l2", l2, nonneg=True)
    _dev_tensors(fname, dev, ((lse, "lse", torch.float32, (N,), False), (loss, "loss", torch.float32, (N,), True)),
                 host_error=ValueError, dtype_error=ValueError)
    o = tuple(out) if out is not None else (None, None, None)
    if len(o) not in (2, 3):
        raise ValueError(f"{fname}: out must be (dW, db) or (dW, db, objective)")
    dW = _out(fname, o[0], "dW", torch.float32, (C, D), dev)
    db = _out(fname, o[1], "db", torch.float32, (C,), dev)
    obj = None
    if loss is not None:
        obj = _out(fname, o[2] if len(o) == 3 else None, "objective", torch.float32, (1,), dev)
    elif len(o) == 3 and o[2] is not None:
        raise ValueError(f"{fname}: an objective output needs `loss`")
    nbytes = probe_workspace(N, C, D)
    ws = _workspace(fname, None, nbytes, torch.float32, dev)
    fn = _fn("cclip_probe_backward", x)
    check(fn(_p(x), c_long(ldx), c_long(N), c_int(D), _p(W), _p(bias), c_int(C), _p(labels), _p(row_weight), _p(lse), _p(loss),
             c_float(scale), c_float(l2), _p(dW), _p(db), _p(obj), _p(ws), c_long(nbytes), _stream()), "cclip_probe_backward")
    return dW, db, obj


TSNE_MAX_K = 63            # one less than similarity_topk's 64: the kNN graph asks for k + 1 and drops the row itself
TSNE_TILE = 512            # points of y per LDS tile of the repulsion kernel
TSNE_SPLIT_MAX = 16        # the most splits of its j range
TSNE_BISECT_STEPS = 100


def _rows_int32(fname: str, N: int) -> int:
    if N < 1:
        raise ValueError(f"{fname}: empty operand (N = {N})")
    if N >= 2 ** 31:
        raise NotImplementedError(f"{fname}: N = {N}; the kernel's row index is int32 (N < 2^31)")
    return N


def tsne_affinities(scores, perplexity: float, *, out_P=None, out_beta=None):
    """The conditional neighbour probabilities of t-SNE (include/cclip_hip.h, cclip_tsne_affinities): scores fp32 [N, k], the
    similarities of every row's k nearest other unit rows (inner stride 1; a row-strided view is fine), 1 <= k <= 63,
    1 < perplexity < k.  Returns (P fp32 [N, k] with rows summing to 1, beta fp32 [N]): beta by 100 fixed bisection steps so
    that the row's entropy is log(perplexity).  One launch; no host read."""
    fname = "tsne_affinities"
    _dev_tensor(fname, scores, "scores", torch.float32, None, None, contiguous=False)
    if scores.dim() != 2 or scores.stride(1) != 1:
        raise ValueError(f"{fname}: scores must be a 2-D view with inner stride 1, got {tuple(scores.shape)} / {scores.stride()}")
    N, k = scores.shape
    if not 1 <= k <= TSNE_MAX_K:
        raise ValueError(f"{fname}: k = {k} outside the kernel's range 1 .. {TSNE_MAX_K}")
    _rows_int32(fname, N)
    perplexity = float(perplexity)
    if not 1.0 < perplexity < k:
        raise ValueError(f"{fname}: perplexity = {perplexity} must lie inside (1, k = {k})")
    ld = _ld(scores, multiple=1, at_least=k)
    if ld < k:
        raise ValueError(f"{fname}: row stride {ld} below k = {k}")
    dev = scores.device
    out_P = _out(fname, out_P, "out_P", torch.float32, (N, k), dev)
    out_beta = _out(fname, out_beta, "out_beta", torch.float32, (N,), dev)
    check(lib.cclip_tsne_affinities(_p(scores), c_long(ld), c_long(N), c_int(k), c_float(perplexity), _p(out_P), _p(out_beta),
                                    _stream()), "cclip_tsne_affinities")
    return out_P, out_beta


def tsne_repulsion_splits(N: int) -> int:
    """the number of runs the repulsion kernel cuts its j range into: a function of N alone (0 for an N it would refuse)"""
    return _query("cclip_tsne_repulsion_splits", c_int, c_long(N))


def tsne_repulsion_workspace(N: int) -> int:
    """bytes of per-(split, row) partials cclip_tsne_repulsion needs ((3 N splits + ceil(N / 256)) * 4; 0 for an N it would refuse)"""
    return _query("cclip_tsne_repulsion_workspace", c_long, c_long(N))


def tsne_repulsion(y, *, out_zrow=None, out_rep=None, out_z=None, workspace=None):
    """The N-body sums of t-SNE (include/cclip_hip.h, cclip_tsne_repulsion): y fp32 [N, 2] contiguous.  With
    w_ij = 1 / (1 + |y_i - y_j|^2) over all j != i, returns (zrow fp32 [N] = sum_j w_ij, rep fp32 [N, 2] = sum_j w_ij^2
    (y_i - y_j), z fp32 [1] = sum_i zrow[i]).  No N x N matrix, no float atomics: two calls are bitwise equal.  `workspace`: a
    float32 device vector of at least tsne_repulsion_workspace(N) bytes to reuse.  Three launches; no host read."""
    fname = "tsne_repulsion"
    N = _rows_int32(fname, _dev_tensor(fname, y, "y", torch.float32, (None, 2), None).shape[0])
    dev = y.device
    out_zrow = _out(fname, out_zrow, "out_zrow", torch.float32, (N,), dev)
    out_rep = _out(fname, out_rep, "out_rep", torch.float32, (N, 2), dev)
    out_z = _out(fname, out_z, "out_z", torch.float32, (1,), dev)
    workspace = _workspace(fname, workspace, tsne_repulsion_workspace(N), torch.float32, dev, flat=True, host_error=TypeError)
    check(lib.cclip_tsne_repulsion(_p(y), c_long(N), _p(out_zrow), _p(out_rep), _p(out_z), _p(workspace),
                                   c_long(workspace.numel() * 4), _stream()), "cclip_tsne_repulsion")
    return out_zrow, out_rep, out_z


def _csr(fname: str, N: int, dev, offsets, cols, vals, *, int32_nnz: bool) -> int:
    """A graph over N rows as CSR: offsets int64 [N + 1], cols int32 [nnz], vals fp32 [nnz], contiguous on dev.  Returns nnz;
    int32_nnz: for a kernel whose entry index is int32."""
    _dev_tensors(fname, dev, ((offsets, "offsets", torch.int64, (N + 1,), False), (cols, "cols", torch.int32, 1, False),
                              (vals, "vals", torch.float32, 1, False)))
    nnz = cols.numel()
    if vals.numel() != nnz:
        raise ValueError(f"{fname}: cols has {nnz} entries, vals {vals.numel()}")
    if int32_nnz and (N >= 2 ** 31 or nnz >= 2 ** 31):
        raise NotImplementedError(f"{fname}: N = {N}, nnz = {nnz}; the kernel's indices are int32 (both < 2^31)")
    return nnz


def tsne_step(y, vel, gains, offsets, cols, vals, rep, z, *, exaggeration: float = 1.0, momentum: float = 0.8,
              learning_rate: float = 200.0, min_gain: float = 0.01, out_y=None, out_kl=None, update: bool = True):
    """One gradient-descent update of t-SNE (include/cclip_hip.h, cclip_tsne_step): y, vel, gains, rep fp32 [N, 2], the joint
    probabilities as CSR (offsets int64 [N + 1], cols int32 [nnz], vals fp32 [nnz]), z the fp32 [1] device scalar of
    tsne_repulsion for this y.  vel and gains are updated in place; returns (y_out, kl_row): y_out = y + vel in a buffer other
    than y, kl_row fp32 [N] the rows' KL terms with the un-exaggerated P.  update=False only evaluates kl_row (vel, gains and
    rep may be None; y_out is None).  One launch; no host read."""
    fname = "tsne_step"
    N = _rows_int32(fname, _dev_tensor(fname, y, "y", torch.float32, (None, 2), None).shape[0])
    dev = y.device
    nnz = _csr(fname, N, dev, offsets, cols, vals, int32_nnz=False)
    _dev_tensor(fname, z, "z", torch.float32, (1,), dev)
    exaggeration, momentum, learning_rate, min_gain = (_finite(fname, n, v, nonneg=True) for n, v in (
        ("exaggeration", exaggeration), ("momentum", momentum), ("learning_rate", learning_rate), ("min_gain", min_gain)))
    if update:
        _dev_tensors(fname, dev, [(t, n, torch.float32, (N, 2), False) for t, n in ((vel, "vel"), (gains, "gains"), (rep, "rep"))])
        out_y = _out(fname, out_y, "out_y", torch.float32, (N, 2), dev)
        if out_y.data_ptr() == y.data_ptr():
            raise ValueError(f"{fname}: out_y must not be y: other rows still read y")
    else:
        if out_y is not None:
            raise ValueError(f"{fname}: update=False writes no out_y")
        vel = gains = rep = None
    out_kl = _out(fname, out_kl, "out_kl", torch.float32, (N,), dev)
    check(lib.cclip_tsne_step(_p(y), _p(vel), _p(gains), c_long(N), _p(offsets), _p(cols), _p(vals), c_long(nnz), _p(rep), _p(z),
                              c_float(exaggeration), c_float(momentum), c_float(learning_rate), c_float(min_gain), _p(out_y),
                              _p(out_kl), _stream()), "cclip_tsne_step")
    return out_y, out_kl


LABEL_SPREAD_MAX_C = 1024


def label_spread_groups(C: int) -> int:
    """the number of edge groups a row's entries are dealt over in label_spread_step: a function of C alone (0 for a C it would refuse)"""
    return _query("cclip_label_spread_groups", c_int, c_int(C))


def label_graph_normalize(offsets, cols, vals, *, out_deg=None, out_vals=None):
    """The normalised graph operator of label spreading (include/cclip_hip.h, cclip_label_graph_normalize): a symmetric
    non-negative graph as CSR (offsets int64 [N + 1], cols int32 [nnz], vals fp32 [nnz]).  Returns (deg fp32 [N], the row
    sums; vals_out fp32 [nnz] = (vals r_i) r_j with r = 1 / sqrt(deg), 0 where deg is not > 0).  out_vals may be `vals`.
    Two launches; no host read."""
    fname = "label_graph_normalize"
    _dev_tensor(fname, offsets, "offsets", None, None, None, contiguous=False)
    N, dev = offsets.numel() - 1, offsets.device
    if N < 1:
        raise ValueError(f"{fname}: empty operand (N = {N})")
    nnz = _csr(fname, N, dev, offsets, cols, vals, int32_nnz=True)
    out_deg = _out(fname, out_deg, "out_deg", torch.float32, (N,), dev)
    out_vals = _out(fname, out_vals, "out_vals", torch.float32, (nnz,), dev)
    check(lib.cclip_label_graph_normalize(_p(offsets), _p(cols), _p(vals), c_long(N), c_long(nnz), _p(out_deg), _p(out_vals),
                                          _stream()), "cclip_label_graph_normalize")
    return out_deg, out_vals


def _label_F(fname: str, F):
    _dev_tensors(fname, None, ((F, "F", torch.float32, 2, False),))
    N, C = F.shape
    if not 2 <= C <= LABEL_SPREAD_MAX_C:
        raise ValueError(f"{fname}: C = {C} outside the kernel's range 2 .. {LABEL_SPREAD_MAX_C}")
    return _rows_int32(fname, N), C


def label_spread_step(F, labels, offsets, cols, vals, alpha: float, class_weight=None, *, out_F=None, out_delta=None,
                      delta: bool = True):
    """One iteration of label spreading (include/cclip_hip.h, cclip_label_spread_step): F fp32 [N, C] contiguous, labels int32
    [N] (< 0 or >= C: unlabelled), S as CSR (label_graph_normalize's vals), class_weight fp32 [C] or None.  Returns (F_out,
    delta_row): F_out = alpha S F + (1 - alpha) Y in a buffer other than F, delta_row fp32 [N] = max_c |F_out - F| (None with
    delta=False).  No float atomics, one fixed order: two calls are bitwise equal.  One launch; no host read."""
    fname = "label_spread_step"
    N, C = _label_F(fname, F)
    dev = F.device
    nnz = _csr(fname, N, dev, offsets, cols, vals, int32_nnz=True)
    _dev_tensors(fname, dev, ((labels, "labels", torch.int32, (N,), False), (class_weight, "class_weight", torch.float32, (C,), True)))
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{fname}: alpha = {alpha} outside [0, 1]")
    out_F = _out(fname, out_F, "out_F", torch.float32, (N, C), dev)
    if out_F.data_ptr() == F.data_ptr():
        raise ValueError(f"{fname}: out_F must not be F: other rows still read F")
    if delta:
        out_delta = _out(fname, out_delta, "out_delta", torch.float32, (N,), dev)
    elif out_delta is not None:
        raise ValueError(f"{fname}: delta=False writes no out_delta")
    check(lib.cclip_label_spread_step(_p(F), _p(out_F), c_long(N), c_int(C), _p(labels), _p(class_weight), _p(offsets), _p(cols),
                                      _p(vals), c_long(nnz), c_float(alpha), _p(out_delta), _stream()), "cclip_label_spread_step")
    return out_F, out_delta


def label_spread_finish(F, *, out_dist=None, out_pred=None, out_conf=None, out_cert=None, dist: bool = True):
    """The read-out of label spreading (include/cclip_hip.h, cclip_label_spread_finish): F fp32 [N, C] contiguous.  Returns
    (dist fp32 [N, C] = F / row sum, None with dist=False; pred int32 [N], the argmax of F, ties to the lowest class; conf fp32
    [N] = max of the dist row; cert fp32 [N] = 1 - H(dist row) / log C).  A row that sums to 0: pred -1, conf = cert = 0, dist
    row 0.  One launch; no host read."""
    fname = "label_spread_finish"
    N, C = _label_F(fname, F)
    dev = F.device
    if dist:
        out_dist = _out(fname, out_dist, "out_dist", torch.float32, (N, C), dev)
    elif out_dist is not None:
        raise ValueError(f"{fname}: dist=False writes no out_dist")
    out_pred = _out(fname, out_pred, "out_pred", torch.int32, (N,), dev)
    out_conf = _out(fname, out_conf, "out_conf", torch.float32, (N,), dev)
    out_cert = _out(fname, out_cert, "out_cert", torch.float32, (N,), dev)
    check(lib.cclip_label_spread_finish(_p(F), c_long(N), c_int(C), _p(out_dist), _p(out_pred), _p(out_conf), _p(out_cert),
                                        _stream()), "cclip_label_spread_finish")
    return out_dist, out_pred, out_conf, out_cert


SAMPLE_ROWS_MAX_V = 65536


def sample_rows(logits, u, done_i32, *, inv_temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, stop_token: int = -1,
                token=None, logprob=None, n_kept=None, kept_mass=None):
    """One sampled token per row (include/cclip_hip.h, cclip_sample_rows): logits fp32 [n, V] with inner stride 1, u fp32 [n]
    uniforms in [0, 1), done_i32 int32 [n] (read, and set to 1 on the rows that draw stop_token; a row entered as done gets
    token 0 at logprob 0).  The logits are multiplied by inv_temperature; top_k = 0 and top_p = 1 switch the filters off.  Returns (token int32, logprob fp32, n_kept int32,
    kept_mass fp32), each [n].  V <= 65536.  One launch; no host read; two calls are bitwise equal."""
    if not 0.0 < inv_temperature < float("inf"):
        raise ValueError(f"sample_rows: inv_temperature must be a positive finite number, got {inv_temperature}")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"sample_rows: top_k must be an integer >= 0 (0 = off), got {top_k}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"sample_rows: top_p must lie in (0, 1] (1 = off), got {top_p}")
    if logits.dtype != torch.float32 or u.dtype != torch.float32:
        raise ValueError(f"sample_rows: logits and u must be float32, got {logits.dtype} / {u.dtype}")
    if done_i32.dtype != torch.int32:
        raise ValueError(f"sample_rows: done must be int32, got {done_i32.dtype}")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError(f"sample_rows: logits must be a 2-D view with inner stride 1, got {tuple(logits.shape)} / {logits.stride()}")
    n, V = logits.shape
    if n < 1 or not 1 <= V <= SAMPLE_ROWS_MAX_V:
        raise ValueError(f"sample_rows: n = {n}, V = {V}; the kernel needs n >= 1 and 1 <= V <= {SAMPLE_ROWS_MAX_V}")
    ld = logits.stride(0) if n > 1 else max(V, logits.stride(0))
    if ld < V:
        raise ValueError(f"sample_rows: row stride {ld} below V = {V}")
    for t, name in ((u, "u"), (done_i32, "done")):
        if tuple(t.shape) != (n,) or not t.is_contiguous() or t.device != logits.device:
            raise ValueError(f"sample_rows: {name} must be a contiguous [{n}] vector on {logits.device}, got {tuple(t.shape)} on {t.device}")
    if not logits.is_cuda:
        raise TypeError(f"sample_rows: expected cuda tensors, got {logits.device} (no CPU path)")
    dev = logits.device
    outs = []
    for t, name, dt in ((token, "token", torch.int32), (logprob, "logprob", torch.float32), (n_kept, "n_kept", torch.int32),
                        (kept_mass, "kept_mass", torch.float32)):
        if t is None:
            t = torch.empty(n, device=dev, dtype=dt)
        if t.dtype != dt or t.device != dev or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"sample_rows: {name} must be a contiguous {dt} [{n}] vector on {dev}, got {t.dtype} {tuple(t.shape)}")
        outs.append(t)
    check(lib.cclip_sample_rows(_p(logits), c_long(ld), c_int(n), c_int(V), c_float(inv_temperature), c_int(min(int(top_k), 2 ** 31 - 1)),
                                c_float(top_p), _p(u), c_int(stop_token), _p(done_i32), _p(outs[0]), _p(outs[1]), _p(outs[2]),
                                _p(outs[3]), _stream()), "cclip_sample_rows")
    return tuple(outs)


CAPTION_SELECT_MAX_K = 64
CAPTION_SELECT_MAX_E = 1024


def _ref_offsets(ref_off, N: int, Rtot: int) -> torch.Tensor:
    """The CSR offsets of caption_select's references, validated on the host: int32 [N + 1] from 0, never decreasing, ending
    inside the Rtot rows (the kernel reads them on the device and trusts them)."""
    if isinstance(ref_off, torch.Tensor):
        if ref_off.is_cuda:
            raise TypeError("caption_select: ref_off must be a host tensor or a sequence (it is validated before the upload)")
        if ref_off.is_floating_point() or ref_off.dim() != 1:
            raise ValueError(f"caption_select: ref_off must be a 1-D integer vector, got {tuple(ref_off.shape)} {ref_off.dtype}")
        off = [int(v) for v in ref_off.tolist()]
    else:
        off = [int(v) for v in ref_off]
    if len(off) != N + 1:
        raise ValueError(f"caption_select: ref_off needs N + 1 = {N + 1} entries, got {len(off)}")
    if off[0] != 0 or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"caption_select: ref_off must start at 0 and never decrease, got {off}")
    if off[-1] > Rtot:
        raise ValueError(f"caption_select: ref_off ends at {off[-1]}, ref has {Rtot} rows")
    return torch.tensor(off, dtype=torch.int32)


def caption_select(img, txt, K: int, *, lm_mean=None, ref=None, ref_off=None, w: float = 2.5, lm_weight: float = 0.0,
                   cos=None, clip_score=None, ref_score=None, score=None, order=None, best=None):
    """K candidate captions per image scored and ranked (include/cclip_hip.h, cclip_caption_select): img fp32 [N, E], txt fp32
    [N * K, E] (row n * K + k = candidate k of image n), both raw tower outputs with inner stride 1, row strides multiples of
    4 floats, 16-byte aligned.  lm_mean fp32 [N * K]: the candidates' mean token log-probability (None = 0).  ref fp32 [Rtot, E]
    with ref_off, N + 1 CSR offsets ON THE HOST (a sequence or a CPU integer tensor; validated here, then uploaded): image n's
    reference captions are rows ref_off[n] .. ref_off[n + 1] - 1, possibly none.  Returns (cos, clip_score, ref_score or None,
    score, order, best): fp32 [N, K] x 4, int32 [N, K], int32 [N]; clip_score = w max(cos, 0), score = cos + lm_weight lm_mean,
    order by (score descending, k ascending).  1 <= K <= 64, E % 4 == 0, E <= 1024.  One launch; no host read; two calls are
    bitwise equal."""
    for t, n in ((img, "img"), (txt, "txt")) + (((ref, "ref"),) if ref is not None else ()):
        if t.dtype != torch.float32:
            raise ValueError(f"caption_select: {n} must be float32, got {t.dtype}")
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"caption_select: {n} must be a 2-D view with inner stride 1, got {tuple(t.shape)} / {t.stride()}")
    N, E = img.shape
    if int(K) != K or K < 1:
        raise ValueError(f"caption_select: K must be an integer >= 1, got {K}")
    K = int(K)
    if N < 1:
        raise ValueError("caption_select: need at least one image")
    if tuple(txt.shape) != (N * K, E):
        raise ValueError(f"caption_select: txt must be [N * K, E] = [{N * K}, {E}], got {tuple(txt.shape)}")
    if (ref is None) != (ref_off is None):
        raise ValueError("caption_select: give both ref and ref_off, or neither")
    if ref is not None and ref.shape[1] != E:
        raise ValueError(f"caption_select: ref has {ref.shape[1]} columns, img has {E}")
    if lm_mean is not None and (lm_mean.dtype != torch.float32 or tuple(lm_mean.shape) != (N * K,) or not lm_mean.is_contiguous()):
        raise ValueError(f"caption_select: lm_mean must be a contiguous float32 [{N * K}] vector, got {lm_mean.dtype} {tuple(lm_mean.shape)}")
    if K > CAPTION_SELECT_MAX_K:
        raise NotImplementedError(f"caption_select: K = {K}; the kernel ranks at most {CAPTION_SELECT_MAX_K} candidates per image")
    if E < 4 or E % 4 or E > CAPTION_SELECT_MAX_E:
        raise NotImplementedError(f"caption_select: E = {E}; the kernel needs E % 4 == 0 and 4 <= E <= {CAPTION_SELECT_MAX_E}")
    off = None if ref_off is None else _ref_offsets(ref_off, N, ref.shape[0])
    if ref is not None and ref.shape[0] == 0:             # no reference anywhere: every rmax is 0, no row is read
        ref = ref.new_zeros(1, E)
    dev = img.device
    lds = []
    for t, n in ((img, "img"), (txt, "txt"), (ref, "ref")):
        if t is None:
            lds.append(E)
            continue
        if not t.is_cuda or t.device != dev:
            raise TypeError(f"caption_select: {n}: expected a cuda tensor on {dev}, got {t.device} (no CPU path)")
        ld = t.stride(0) if t.shape[0] > 1 else max(E, t.stride(0) // 4 * 4)
        if ld < E or ld % 4 or t.data_ptr() % 16:
            raise ValueError(f"caption_select: {n} must be 16-byte aligned with a row stride >= E that is a multiple of 4 floats "
                             f"(stride {t.stride(0)}, address % 16 = {t.data_ptr() % 16})")
        lds.append(ld)
    if lm_mean is not None and lm_mean.device != dev:
        raise TypeError(f"caption_select: lm_mean: expected a tensor on {dev}, got {lm_mean.device}")
    outs = []
    for t, n, dt, shape in ((cos, "cos", torch.float32, (N, K)), (clip_score, "clip_score", torch.float32, (N, K)),
                            (ref_score, "ref_score", torch.float32, (N, K)), (score, "score", torch.float32, (N, K)),
                            (order, "order", torch.int32, (N, K)), (best, "best", torch.int32, (N,))):
        if n == "ref_score" and ref is None:
            if t is not None:
                raise ValueError("caption_select: ref_score given without references")
            outs.append(None)
            continue
        if t is None:
            t = torch.empty(shape, device=dev, dtype=dt)
        if t.dtype != dt or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"caption_select: {n} must be a contiguous {dt} {list(shape)} tensor on {dev}, got {t.dtype} {tuple(t.shape)}")
        outs.append(t)
    off_dev = None if off is None else off.to(dev)
    check(lib.cclip_caption_select(_p(img), c_long(lds[0]), _p(txt), c_long(lds[1]), c_int(N), c_int(K), c_int(E), _p(lm_mean), _p(ref),
                                   c_long(lds[2]), _p(off_dev), c_float(w), c_float(lm_weight), _p(outs[0]), _p(outs[1]), _p(outs[2]),
                                   _p(outs[3]), _p(outs[4]), _p(outs[5]), _stream()), "cclip_caption_select")
    return tuple(outs)


def attention_small_fwd(q, k, v, o, *, B: int, T: int, H: int, head_dim: int, lse=None, scale=None) -> None:
    """Generic-head_dim unmasked attention (TransformerMapper): same tensor conventions as attention_fwd."""
    d = _attn_desc(q, k, v, o, lse, B, T, H, False, None, scale, head_dim)
    check(_fn("cclip_attention_small_fwd", q, k, v, o)(ctypes.byref(d), _stream()), "cclip_attention_small_fwd")


def attention_small_bwd(q, k, v, o, lse, dout, dq, dk, dv, *, B: int, T: int, H: int, head_dim: int, scale=None) -> None:
    d = _attn_desc(q, k, v, o, lse, B, T, H, False, None, scale, head_dim)
    _attn_grads(d, dout, dq, dk, dv)
    check(_fn("cclip_attention_small_bwd", q, k, v, o, dout, dq, dk, dv)(ctypes.byref(d), _stream()), "cclip_attention_small_bwd")


def attention_decode(q, kcache, vcache, out, *, H: int, S: int, scale=None) -> None:
    """One new query per sequence against its KV cache.  q/out: [B, H*64] 16-bit rows (any row stride); kcache/vcache:
    [B, Smax, H*64] views (position stride = stride(1), sequence stride = stride(0)); S = cached positions incl. the new one."""
    for t, n in ((q, "q"), (kcache, "kcache"), (vcache, "vcache"), (out, "out")):
        _req16(t, n)
        assert t.stride(-1) == 1
    B = q.shape[0]
    assert kcache.dim() == 3 and vcache.shape == kcache.shape and kcache.stride() == vcache.stride() and S <= kcache.shape[1]
    check(_fn("cclip_attention_decode", q, kcache, vcache, out)(
        _p(q), c_long(q.stride(0)), _p(kcache), _p(vcache), c_long(kcache.stride(1)), c_long(kcache.stride(0)), _p(out),
        c_long(out.stride(0)), c_int(B), c_int(H), c_int(S), c_float(64 ** -0.5 if scale is None else scale), _stream()),
        "cclip_attention_decode")


# --------------------------------------------------------------------------------------------
# device-side preprocess (PIL's 8-bit bicubic resampler + crop + normalise)
# --------------------------------------------------------------------------------------------
def resample_h_u8(src_rows: torch.Tensor, bounds: torch.Tensor, kk: torch.Tensor, ksize: int, out: torch.Tensor) -> None:
    """src_rows uint8 [rows, W, 3] -> out uint8 [rows, n, 3]; bounds int32 [n, 2], kk int32 [n, ksize]."""
    assert src_rows.dtype == torch.uint8 and out.dtype == torch.uint8 and src_rows.is_cuda and src_rows.stride(2) == 1 and src_rows.stride(1) == 3
    assert bounds.dtype == torch.int32 and kk.dtype == torch.int32 and bounds.is_contiguous() and kk.is_contiguous() and out.is_contiguous()
    check(lib.cclip_resample_h_u8(_p(src_rows), c_long(src_rows.stride(0)), c_int(src_rows.shape[0]), _p(bounds), _p(kk), c_int(ksize),
                                  c_int(out.shape[1]), _p(out), c_long(out.stride(0)), _stream()), "cclip_resample_h_u8")


def resample_v_norm(tmp: torch.Tensor, row0: int, bounds: torch.Tensor, kk: torch.Tensor, ksize: int, mean, std, out: torch.Tensor) -> None:
    """tmp uint8 [rows, n, 3] (input rows row0..) -> out fp32 [3, n, n] = ((u8 / 255) - mean) / std."""
    _req(out, torch.float32, "out")
    assert tmp.dtype == torch.uint8 and tmp.is_contiguous() and out.is_contiguous()
    m3, s3 = (c_float * 3)(*mean), (c_float * 3)(*std)
    check(lib.cclip_resample_v_norm(_p(tmp), c_long(tmp.stride(0)), c_int(row0), _p(bounds), _p(kk), c_int(ksize), c_int(out.shape[1]),
                                    m3, s3, _p(out), _stream()), "cclip_resample_v_norm")


# region preprocess: K boxes in three launches, tables built on the device (csrc/preprocess_rois.hip).  `desc_host` / `desc`:
# the same int64 [K, ROI_DESC_FIELDS] records (cclip_roi_desc) on the host, where the launcher checks them, and on the device.
ROI_DESC_FIELDS = 11
ROI_MAX_KSIZE = 257


def _roi_args(desc_host: torch.Tensor, desc: torch.Tensor, n: int, ksize_max: int, bounds: torch.Tensor, kk: torch.Tensor) -> int:
    if desc_host.is_cuda or desc_host.dtype != torch.int64:
        raise TypeError(f"desc_host: expected cpu torch.int64, got {desc_host.device} {desc_host.dtype}")
    _req(desc, torch.int64, "desc"); _req(bounds, torch.int32, "bounds"); _req(kk, torch.int32, "kk")
    K = desc_host.shape[0]
    assert desc_host.shape == (K, ROI_DESC_FIELDS) and desc.shape == (K, ROI_DESC_FIELDS) and desc_host.is_contiguous() and desc.is_contiguous()
    assert bounds.shape == (K, 2, n, 2) and kk.shape == (K, 2, n, ksize_max) and bounds.is_contiguous() and kk.is_contiguous()
    return K


def roi_coeffs(desc_host: torch.Tensor, desc: torch.Tensor, n: int, ksize_max: int, bounds: torch.Tensor, kk: torch.Tensor) -> None:
    """Fills bounds int32 [K, 2, n, 2] and kk int32 [K, 2, n, ksize_max] with PIL's windows and coefficients of every box."""
    K = _roi_args(desc_host, desc, n, ksize_max, bounds, kk)
    check(lib.cclip_roi_coeffs(_p(desc_host), _p(desc), c_int(K), c_int(n), c_int(ksize_max), _p(bounds), _p(kk), _stream()),
          "cclip_roi_coeffs")


def roi_resample_h(src: torch.Tensor, desc_host: torch.Tensor, desc: torch.Tensor, n: int, ksize_max: int, bounds: torch.Tensor,
                   kk: torch.Tensor, tmp: torch.Tensor) -> None:
    """src uint8 (flat, every photo of the call) -> tmp uint8 (flat): the horizontal pass of every box over the rows it needs."""
    _req(src, torch.uint8, "src"); _req(tmp, torch.uint8, "tmp")
    K = _roi_args(desc_host, desc, n, ksize_max, bounds, kk)
    assert src.is_contiguous() and tmp.is_contiguous()
    check(lib.cclip_roi_resample_h(_p(src), c_long(src.numel()), _p(desc_host), _p(desc), c_int(K), c_int(n), c_int(ksize_max), _p(bounds),
                                   _p(kk), _p(tmp), c_long(tmp.numel()), _stream()), "cclip_roi_resample_h")


def roi_resample_v_norm(tmp: torch.Tensor, desc_host: torch.Tensor, desc: torch.Tensor, n: int, ksize_max: int, bounds: torch.Tensor,
                        kk: torch.Tensor, mean, std, out: torch.Tensor) -> None:
    """tmp uint8 (flat) -> out fp32 [K, 3, n, n] = ((u8 / 255) - mean) / std of the vertical pass, cropped."""
    _req(tmp, torch.uint8, "tmp"); _req(out, torch.float32, "out")
    K = _roi_args(desc_host, desc, n, ksize_max, bounds, kk)
    assert tmp.is_contiguous() and out.is_contiguous() and out.shape == (K, 3, n, n)
    m3, s3 = (c_float * 3)(*mean), (c_float * 3)(*std)
    check(lib.cclip_roi_resample_v_norm(_p(tmp), c_long(tmp.numel()), _p(desc_host), _p(desc), c_int(K), c_int(n), c_int(ksize_max),
                                        _p(bounds), _p(kk), m3, s3, _p(out), _stream()), "cclip_roi_resample_v_norm")


OVERLAY_MAX_SIDE = 16384


def _cuda_operands(fname: str, tensors, ref: torch.Tensor, strided=()) -> None:
    """The operand contract of the overlay and dense-map wrappers: cuda tensor, dtype, contiguous (row-strided for the names in
    `strided`), on `ref`'s device - each refusal a ValueError that names the operand."""
    for t, name, dt in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{fname}: {name} must be a cuda tensor, got {getattr(t, 'device', type(t))} (no CPU path)")
        if t.dtype != dt:
            raise ValueError(f"{fname}: {name} must be {dt}, got {t.dtype}")
        if name in strided:
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{fname}: {name} must be 2-D with inner stride 1, got shape {tuple(t.shape)} strides {t.stride()}")
        elif not t.is_contiguous():
            raise ValueError(f"{fname}: {name} must be contiguous, got shape {tuple(t.shape)} strides {t.stride()}")
        if t.device != ref.device:
            raise ValueError(f"{fname}: {name} is on {t.device}, {tensors[0][1]} on {ref.device}")


def relevance_overlay(rel: torch.Tensor, images: torch.Tensor, lut: torch.Tensor, size: int, out: torch.Tensor,
                      map_out: Optional[torch.Tensor] = None) -> None:
    """N relevance overlays in one launch (include/cclip_hip.h, cclip_relevance_overlay): rel fp32 [N, g*g], images fp32
    [N, 3, R, R] or [1, 3, R, R] (one image under all N maps), lut fp32 [256, 3] -> out uint8 [>= N, size, size, 3] (the first N
    overlays are written) and, when given, map_out fp32 [N, size, size] (the min-max normalised upsampled map).  All contiguous
    cuda tensors on one device; no CPU path.  Two calls give equal bytes."""
    tensors = [(rel, "rel", torch.float32), (images, "images", torch.float32), (lut, "lut", torch.float32), (out, "out", torch.uint8)]
    if map_out is not None:
        tensors.append((map_out, "map_out", torch.float32))
    _cuda_operands("relevance_overlay", tensors, rel)
    if rel.dim() != 2 or rel.shape[0] < 1:
        raise ValueError(f"relevance_overlay: rel must be [N, g*g] with N >= 1, got {tuple(rel.shape)}")
    N, P = rel.shape
    g = int(round(P ** 0.5))
    if g < 1 or g * g != P:
        raise ValueError(f"relevance_overlay: {P} patches do not form a square grid")
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3] or images.shape[2] < 1:
        raise ValueError(f"relevance_overlay: images must be [N, 3, R, R], got {tuple(images.shape)}")
    if images.shape[0] not in (1, N):
        raise ValueError(f"relevance_overlay: {images.shape[0]} images for {N} maps (give one image, or one per map)")
    R = images.shape[2]
    if int(size) != size or not 1 <= size <= OVERLAY_MAX_SIDE or max(g, R) > OVERLAY_MAX_SIDE:
        raise ValueError(f"relevance_overlay: size {size}, grid {g}, resolution {R}: each must lie in [1, {OVERLAY_MAX_SIDE}]")
    size = int(size)
    if tuple(lut.shape) != (256, 3):
        raise ValueError(f"relevance_overlay: lut must be [256, 3], got {tuple(lut.shape)}")
    if out.dim() != 4 or out.shape[0] < N or tuple(out.shape[1:]) != (size, size, 3):
        raise ValueError(f"relevance_overlay: out must be [>= {N}, {size}, {size}, 3], got {tuple(out.shape)}")
    if map_out is not None and tuple(map_out.shape) != (N, size, size):
        raise ValueError(f"relevance_overlay: map_out must be [{N}, {size}, {size}], got {tuple(map_out.shape)}")
    stride = 0 if images.shape[0] == 1 else 3 * R * R
    check(lib.cclip_relevance_overlay(_p(rel), c_int(N), c_int(g), _p(images), c_long(stride), c_int(R), _p(lut), c_int(size), _p(out),
                                      _p(map_out), _stream()), "cclip_relevance_overlay")


DENSE_MAX_CLASSES, DENSE_MAX_EMBED = 255, 1024


def dense_class_probs(feat: torch.Tensor, text: torch.Tensor, scale: float, patches: int, probs: torch.Tensor,
                      logits_out: Optional[torch.Tensor] = None) -> None:
    """Per-patch class probabilities (include/cclip_hip.h, cclip_dense_class_probs): feat fp32 [B * patches, E] (rows may be
    strided), text fp32 [C, E], neither normalised -> probs fp32 [B, C, patches] = softmax over C of scale * cosine, class-major,
    and, when given, logits_out of the same shape.  1 <= C <= 255, E a multiple of 4, <= 1024.  cuda tensors on one device; no
    CPU path.  Two calls give equal bytes."""
    fname = "dense_class_probs"
    tensors = [(feat, "feat", torch.float32), (text, "text", torch.float32), (probs, "probs", torch.float32)]
    if logits_out is not None:
        tensors.append((logits_out, "logits_out", torch.float32))
    _cuda_operands(fname, tensors, feat, strided=("feat",))
    if text.dim() != 2 or text.shape[1] != feat.shape[1]:
        raise ValueError(f"{fname}: text must be [C, {feat.shape[1]}], got {tuple(text.shape)}")
    M, E = feat.shape
    C = text.shape[0]
    if not 1 <= C <= DENSE_MAX_CLASSES:
        raise ValueError(f"{fname}: {C} classes; text must hold between 1 and {DENSE_MAX_CLASSES} rows")
    if E < 4 or E % 4 or E > DENSE_MAX_EMBED:
        raise ValueError(f"{fname}: feat has embedding width {E}; it must be a multiple of 4 in [4, {DENSE_MAX_EMBED}]")
    if int(patches) != patches or patches < 1 or M < 1 or M % patches:
        raise ValueError(f"{fname}: feat has {M} rows, not a positive multiple of patches = {patches}")
    patches = int(patches)
    if M > 1 and (feat.stride(0) < E or feat.stride(0) % 4):
        raise ValueError(f"{fname}: feat must have a row stride >= {E} that is a multiple of 4, got {feat.stride(0)}")
    if feat.data_ptr() % 16 or text.data_ptr() % 16:
        raise ValueError(f"{fname}: feat and text must start on a 16-byte boundary")
    B = M // patches
    if tuple(probs.shape) != (B, C, patches):
        raise ValueError(f"{fname}: probs must be [{B}, {C}, {patches}], got {tuple(probs.shape)}")
    if logits_out is not None and tuple(logits_out.shape) != (B, C, patches):
        raise ValueError(f"{fname}: logits_out must be [{B}, {C}, {patches}], got {tuple(logits_out.shape)}")
    ldf = feat.stride(0) if M > 1 else E
    check(lib.cclip_dense_class_probs(_p(feat), c_long(ldf), c_long(M), c_int(patches), _p(text), c_int(C), c_int(E),
                                      c_float(float(scale)), _p(probs), _p(logits_out), _stream()), "cclip_dense_class_probs")


def _label_outputs(fname: str, shape, labels, conf, cover, overlay, palette, photo, alpha8) -> None:
    """The output side of dense_label_map and dense_stitch, `shape` = (B, S, S) or (H, W): labels, conf and (when given) cover of
    that shape, overlay and photo of that shape + [3], palette [256, 3] with an overlay and neither it nor a photo without,
    alpha8 in [0, 256]."""
    for t, name in ((labels, "labels"), (conf, "conf"), (cover, "cover")):
        if t is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{fname}: {name} must be {list(shape)}, got {tuple(t.shape)}")
    if overlay is None and (photo is not None or palette is not None):
        raise ValueError(f"{fname}: palette and photo are inputs of the overlay; give overlay too")
    if overlay is not None:
        pic = [*shape, 3]
        if palette is None or tuple(palette.shape) != (256, 3):
            raise ValueError(f"{fname}: palette must be uint8 [256, 3], got {None if palette is None else tuple(palette.shape)}")
        if tuple(overlay.shape) != tuple(pic):
            raise ValueError(f"{fname}: overlay must be {pic}, got {tuple(overlay.shape)}")
        if photo is not None and tuple(photo.shape) != tuple(pic):
            raise ValueError(f"{fname}: photo must be {pic} (already at the output size), got {tuple(photo.shape)}")
    if int(alpha8) != alpha8 or not 0 <= alpha8 <= 256:
        raise ValueError(f"{fname}: alpha8 must be an integer in [0, 256], got {alpha8}")


def dense_label_map(probs: torch.Tensor, size: int, labels: torch.Tensor, conf: torch.Tensor, *, min_conf: float = 0.0,
                    overlay: Optional[torch.Tensor] = None, palette: Optional[torch.Tensor] = None,
                    photo: Optional[torch.Tensor] = None, alpha8: int = 256) -> None:
    """Label map and picture of per-patch probabilities (include/cclip_hip.h, cclip_dense_label_map): probs fp32 [B, C, g, g] ->
    labels uint8 [B, size, size] (the lowest arg-max class of the bilinearly upsampled maps, 255 below min_conf), conf fp32
    [B, size, size], and with overlay uint8 [B, size, size, 3]: palette uint8 [256, 3] at the label, blended in integers over
    photo uint8 [B, size, size, 3] with weight alpha8 / 256 when a photo is given.  Contiguous cuda tensors on one device; no CPU
    path.  Two calls give equal bytes."""
    fname = "dense_label_map"
    tensors = [(probs, "probs", torch.float32), (labels, "labels", torch.uint8), (conf, "conf", torch.float32)]
    for t, name in ((overlay, "overlay"), (palette, "palette"), (photo, "photo")):
        if t is not None:
            tensors.append((t, name, torch.uint8))
    _cuda_operands(fname, tensors, probs)
    if probs.dim() != 4 or probs.shape[2] != probs.shape[3] or min(probs.shape) < 1:
        raise ValueError(f"{fname}: probs must be [B, C, g, g] with no empty dimension, got {tuple(probs.shape)}")
    B, C, g, _ = probs.shape
    if C > DENSE_MAX_CLASSES:
        raise ValueError(f"{fname}: probs holds {C} classes; at most {DENSE_MAX_CLASSES} (label 255 means none)")
    if int(size) != size or not 1 <= size <= OVERLAY_MAX_SIDE or g > OVERLAY_MAX_SIDE:
        raise ValueError(f"{fname}: size {size}, grid {g}: each must lie in [1, {OVERLAY_MAX_SIDE}]")
    size = int(size)
    _label_outputs(fname, (B, size, size), labels, conf, None, overlay, palette, photo, alpha8)
    check(lib.cclip_dense_label_map(_p(probs), c_int(B), c_int(C), c_int(g), c_int(size), c_float(float(min_conf)), _p(labels),
                                    _p(conf), _p(palette), _p(photo), c_int(int(alpha8)), _p(overlay), _stream()),
          "cclip_dense_label_map")


DENSE_MAX_WINDOWS = 65535


def _stitch_inputs(fname: str, probs, boxes, height, width):
    """The input side of dense_stitch and dense_stitch_maps: probs [K, C, g, g] inside the window and class caps, boxes [K, 4], and
    height, width and g in [1, OVERLAY_MAX_SIDE]; returns K, C, g, H, W."""
    if probs.dim() != 4 or probs.shape[2] != probs.shape[3] or min(probs.shape) < 1:
        raise ValueError(f"{fname}: probs must be [K, C, g, g] with no empty dimension, got {tuple(probs.shape)}")
    K, C, g, _ = probs.shape
    if K > DENSE_MAX_WINDOWS:
        raise ValueError(f"{fname}: probs holds {K} windows; at most {DENSE_MAX_WINDOWS}")
    if C > DENSE_MAX_CLASSES:
        raise ValueError(f"{fname}: probs holds {C} classes; at most {DENSE_MAX_CLASSES} (label 255 means none)")
    if tuple(boxes.shape) != (K, 4):
        raise ValueError(f"{fname}: boxes must be [{K}, 4] as (x0, y0, x1, y1), got {tuple(boxes.shape)}")
    if int(height) != height or int(width) != width or not 1 <= height <= OVERLAY_MAX_SIDE or not 1 <= width <= OVERLAY_MAX_SIDE \
            or g > OVERLAY_MAX_SIDE:
        raise ValueError(f"{fname}: height {height}, width {width}, grid {g}: each must lie in [1, {OVERLAY_MAX_SIDE}]")
    return K, C, g, int(height), int(width)


def dense_stitch(probs: torch.Tensor, boxes: torch.Tensor, height: int, width: int, labels: torch.Tensor, conf: torch.Tensor, *,
                 min_conf: float = 0.0, cover: Optional[torch.Tensor] = None, overlay: Optional[torch.Tensor] = None,
                 palette: Optional[torch.Tensor] = None, photo: Optional[torch.Tensor] = None, alpha8: int = 256) -> None:
    """Stitch the class maps of K windows into one picture (include/cclip_hip.h, cclip_dense_stitch): probs fp32 [K, C, g, g], map
    set k sampled window-locally over boxes[k] = (x0, y0, x1, y1) (int32 [K, 4], cuda) and averaged, in ascending k, over the
    windows that cover a pixel -> labels uint8 [height, width] (255: below min_conf, or no window), conf fp32 [height, width],
    cover uint8 [height, width] (windows per pixel, saturating) and overlay uint8 [height, width, 3] as dense_label_map makes
    it (palette uint8 [256, 3], photo uint8 [height, width, 3]).  The boxes are NOT read back: an empty, inverted or oversized
    box covers nothing, one that hangs over the edge covers what lies inside, and no box value leads the kernel outside probs.
    Contiguous cuda tensors on one device; no CPU path.  Two calls give equal bytes."""
    fname = "dense_stitch"
    tensors = [(probs, "probs", torch.float32), (boxes, "boxes", torch.int32), (labels, "labels", torch.uint8),
               (conf, "conf", torch.float32)]
    for t, name in ((cover, "cover"), (overlay, "overlay"), (palette, "palette"), (photo, "photo")):
        if t is not None:
            tensors.append((t, name, torch.uint8))
    _cuda_operands(fname, tensors, probs)
    K, C, g, H, W = _stitch_inputs(fname, probs, boxes, height, width)
    _label_outputs(fname, (H, W), labels, conf, cover, overlay, palette, photo, alpha8)
    if probs.data_ptr() % 4 or conf.data_ptr() % 4 or boxes.data_ptr() % 4:
        raise ValueError(f"{fname}: probs, conf and boxes must start on a 4-byte boundary")
    check(lib.cclip_dense_stitch(_p(probs), c_int(K), c_int(C), c_int(g), _p(boxes), c_int(H), c_int(W), c_float(float(min_conf)),
                                 _p(labels), _p(conf), _p(cover), _p(palette), _p(photo), c_int(int(alpha8)), _p(overlay), _stream()),
          "cclip_dense_stitch")


REFINE_MAX_DILATIONS, REFINE_MAX_DILATION, REFINE_DEFAULT_DILATIONS = 6, 24, (1, 2, 4, 8, 12, 24)
_INT32_MAX = 2 ** 31 - 1


def dense_stitch_maps(probs: torch.Tensor, boxes: torch.Tensor, height: int, width: int, maps: torch.Tensor, *,
                      cover: Optional[torch.Tensor] = None) -> None:
    """The stitch's averaged class maps themselves (include/cclip_hip.h, cclip_dense_stitch_maps): probs fp32 [K, C, g, g] and boxes
    int32 [K, 4] as dense_stitch takes them -> maps fp32 [C, height, width] = u_c (0 where no window covers the pixel) and, when
    given, cover uint8 [height, width].  Their maximum over c is dense_stitch's conf, bit for bit.  Contiguous cuda tensors on
    one device; no CPU path.  Two calls give equal bytes."""
    fname = "dense_stitch_maps"
    tensors = [(probs, "probs", torch.float32), (boxes, "boxes", torch.int32), (maps, "maps", torch.float32)]
    if cover is not None:
        tensors.append((cover, "cover", torch.uint8))
    _cuda_operands(fname, tensors, probs)
    K, C, g, H, W = _stitch_inputs(fname, probs, boxes, height, width)
    if C * H * W > _INT32_MAX:
        raise ValueError(f"{fname}: {C} x {H} x {W} map values; at most 2^31 - 1")
    if tuple(maps.shape) != (C, H, W):
        raise ValueError(f"{fname}: maps must be [{C}, {H}, {W}], got {tuple(maps.shape)}")
    if cover is not None and tuple(cover.shape) != (H, W):
        raise ValueError(f"{fname}: cover must be [{H}, {W}], got {tuple(cover.shape)}")
    if probs.data_ptr() % 4 or maps.data_ptr() % 4 or boxes.data_ptr() % 4:
        raise ValueError(f"{fname}: probs, maps and boxes must start on a 4-byte boundary")
    check(lib.cclip_dense_stitch_maps(_p(probs), c_int(K), c_int(C), c_int(g), _p(boxes), c_int(H), c_int(W), _p(maps), _p(cover),
                                      _stream()), "cclip_dense_stitch_maps")


def _refine_maps_shape(fname: str, maps, name: str = "maps"):
    if maps.dim() != 4 or min(maps.shape) < 1:
        raise ValueError(f"{fname}: {name} must be [B, C, H, W] with no empty dimension, got {tuple(maps.shape)}")
    B, C, H, W = maps.shape
    if C > DENSE_MAX_CLASSES:
        raise ValueError(f"{fname}: {name} holds {C} classes; at most {DENSE_MAX_CLASSES} (label 255 means none)")
    if H > OVERLAY_MAX_SIDE or W > OVERLAY_MAX_SIDE:
        raise ValueError(f"{fname}: height {H}, width {W}: each must lie in [1, {OVERLAY_MAX_SIDE}]")
    if B * C * H * W > _INT32_MAX:
        raise ValueError(f"{fname}: {B} x {C} x {H} x {W} map values; at most 2^31 - 1")
    return B, C, H, W


def dense_maps_label(maps: torch.Tensor, labels: torch.Tensor, conf: torch.Tensor, *, min_conf: float = 0.0,
                     cover: Optional[torch.Tensor] = None, overlay: Optional[torch.Tensor] = None,
                     palette: Optional[torch.Tensor] = None, photo: Optional[torch.Tensor] = None, alpha8: int = 256) -> None:
    """Labels, conf and the picture of class maps at the output size (include/cclip_hip.h, cclip_dense_maps_label): maps fp32
    [B, C, H, W] -> labels uint8 [B, H, W] (the lowest arg-max class, 255 below min_conf), conf fp32 [B, H, W] and overlay uint8
    [B, H, W, 3] as dense_label_map makes it.  cover uint8 [B, H, W] is an INPUT: where it is 0 the pixel gets label 255 and conf
    0.  Contiguous cuda tensors on one device; no CPU path.  Two calls give equal bytes."""
    fname = "dense_maps_label"
    tensors = [(maps, "maps", torch.float32), (labels, "labels", torch.uint8), (conf, "conf", torch.float32)]
    for t, name in ((cover, "cover"), (overlay, "overlay"), (palette, "palette"), (photo, "photo")):
        if t is not None:
            tensors.append((t, name, torch.uint8))
    _cuda_operands(fname, tensors, maps)
    B, C, H, W = _refine_maps_shape(fname, maps)
    _label_outputs(fname, (B, H, W), labels, conf, cover, overlay, palette, photo, alpha8)
    if maps.data_ptr() % 4 or conf.data_ptr() % 4:
        raise ValueError(f"{fname}: maps and conf must start on a 4-byte boundary")
    check(lib.cclip_dense_maps_label(_p(maps), c_int(B), c_int(C), c_int(H), c_int(W), _p(cover), c_float(float(min_conf)), _p(labels),
                                     _p(conf), _p(palette), _p(photo), c_int(int(alpha8)), _p(overlay), _stream()),
          "cclip_dense_maps_label")


def refine_dilations(fname: str, dilations) -> tuple:
    """the dilations as a tuple of ints, checked: 1 to 6 of them, each in [1, 24]"""
    try:
        ds = tuple(dilations)
    except TypeError:
        raise ValueError(f"{fname}: dilations must be a sequence of integers, got {dilations!r}") from None
    if not 1 <= len(ds) <= REFINE_MAX_DILATIONS:
        raise ValueError(f"{fname}: {len(ds)} dilations; between 1 and {REFINE_MAX_DILATIONS}")
    for d in ds:
        if isinstance(d, bool) or int(d) != d or not 1 <= d <= REFINE_MAX_DILATION:
            raise ValueError(f"{fname}: dilation {d!r}: each must be an integer in [1, {REFINE_MAX_DILATION}]")
    return tuple(int(d) for d in ds)


def _refine_guide(fname: str, guide, B: int, H: int, W: int) -> None:
    if tuple(guide.shape) != (B, H, W, 3):
        raise ValueError(f"{fname}: guide must be [{B}, {H}, {W}, 3] (the photo at the maps' size), got {tuple(guide.shape)}")


def dense_refine_prepare(guide: torch.Tensor, dilations, key: torch.Tensor) -> None:
    """The per-pixel key of the refinement (include/cclip_hip.h, cclip_dense_refine_prepare): guide uint8 [B, H, W, 3] -> key fp32
    [B, H, W, 4] = the three factors 1 / (1e-8 + 0.1 sigma_k) and the log-normaliser of the 8 D neighbour logits.  Contiguous
    cuda tensors on one device; no CPU path.  Two calls give equal bytes."""
    fname = "dense_refine_prepare"
    ds = refine_dilations(fname, dilations)
    _cuda_operands(fname, [(guide, "guide", torch.uint8), (key, "key", torch.float32)], guide)
    if guide.dim() != 4 or guide.shape[3] != 3 or min(guide.shape) < 1:
        raise ValueError(f"{fname}: guide must be [B, H, W, 3] with no empty dimension, got {tuple(guide.shape)}")
    B, H, W, _ = guide.shape
    if H > OVERLAY_MAX_SIDE or W > OVERLAY_MAX_SIDE or B * H * W > _INT32_MAX:
        raise ValueError(f"{fname}: height {H}, width {W}: each must lie in [1, {OVERLAY_MAX_SIDE}], and B H W <= 2^31 - 1")
    if tuple(key.shape) != (B, H, W, 4):
        raise ValueError(f"{fname}: key must be [{B}, {H}, {W}, 4], got {tuple(key.shape)}")
    if key.data_ptr() % 16:
        raise ValueError(f"{fname}: key must start on a 16-byte boundary")
    check(lib.cclip_dense_refine_prepare(_p(guide), c_int(B), c_int(H), c_int(W), (c_int * len(ds))(*ds), c_int(len(ds)), _p(key),
                                         _stream()), "cclip_dense_refine_prepare")


def dense_refine_step(maps_in: torch.Tensor, maps_out: torch.Tensor, guide: torch.Tensor, key: torch.Tensor, dilations) -> None:
    """One iteration of the refinement (include/cclip_hip.h, cclip_dense_refine_step): maps_out[b, c, p] = sum over the 8 D
    neighbours q_n of p, in ascending n, of exp(a_n(p) - L(p)) maps_in[b, c, q_n], with the guide, the key dense_refine_prepare
    made from it and the same dilations.  maps_in and maps_out fp32 [B, C, H, W], two different buffers.  Contiguous cuda tensors
    on one device; no CPU path.  Two calls give equal bytes."""
    fname = "dense_refine_step"
    ds = refine_dilations(fname, dilations)
    for t, name in ((maps_in, "maps_in"), (maps_out, "maps_out")):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{fname}: {name} must be a [B, C, H, W] tensor, got {tuple(getattr(t, 'shape', ()))}")
    if maps_in is maps_out or (maps_in.device == maps_out.device and maps_in.data_ptr() == maps_out.data_ptr()):
        raise ValueError(f"{fname}: maps_in and maps_out must be two buffers (no in-place step)")
    _cuda_operands(fname, [(maps_in, "maps_in", torch.float32), (maps_out, "maps_out", torch.float32), (guide, "guide", torch.uint8),
                           (key, "key", torch.float32)], maps_in)
    B, C, H, W = _refine_maps_shape(fname, maps_in, "maps_in")
    if tuple(maps_out.shape) != (B, C, H, W):
        raise ValueError(f"{fname}: maps_out must be [{B}, {C}, {H}, {W}], got {tuple(maps_out.shape)}")
    _refine_guide(fname, guide, B, H, W)
    if tuple(key.shape) != (B, H, W, 4):
        raise ValueError(f"{fname}: key must be [{B}, {H}, {W}, 4], got {tuple(key.shape)}")
    n = 4 * maps_in.numel()
    if maps_in.data_ptr() < maps_out.data_ptr() + n and maps_out.data_ptr() < maps_in.data_ptr() + n:
        raise ValueError(f"{fname}: maps_in and maps_out overlap (no in-place step)")
    if maps_in.data_ptr() % 4 or maps_out.data_ptr() % 4 or key.data_ptr() % 16:
        raise ValueError(f"{fname}: the maps must start on a 4-byte boundary, key on a 16-byte boundary")
    check(lib.cclip_dense_refine_step(_p(maps_in), _p(maps_out), _p(guide), _p(key), c_int(B), c_int(C), c_int(H), c_int(W),
                                      (c_int * len(ds))(*ds), c_int(len(ds)), _stream()), "cclip_dense_refine_step")


COMPONENTS_GROUP = 1024


def _component_maps(fname: str, labels, maps):
    """The label map of the component wrappers, uint8 [B, H, W], and the per-pixel maps (t, name, dtype) of the same shape:
    cuda tensor, dtype, contiguous, one device, then the shapes and the size limits.  Returns (B, H, W)."""
    _cuda_operands(fname, [(labels, "labels", torch.uint8)] + [m for m in maps if m[0] is not None], labels)
    if labels.dim() != 3 or min(labels.shape) < 1:
        raise ValueError(f"{fname}: labels must be [B, H, W] with no empty dimension, got {tuple(labels.shape)}")
    B, H, W = labels.shape
    if H > OVERLAY_MAX_SIDE or W > OVERLAY_MAX_SIDE:
        raise ValueError(f"{fname}: height {H}, width {W}: each must lie in [1, {OVERLAY_MAX_SIDE}]")
    if B * H * W > 2 ** 31 - 1:
        raise ValueError(f"{fname}: labels holds {B * H * W} pixels; flat indices are int32, at most {2 ** 31 - 1}")
    for t, name, _ in maps:
        if t is not None and tuple(t.shape) != (B, H, W):
            raise ValueError(f"{fname}: {name} must be {[B, H, W]}, got {tuple(t.shape)}")
    return B, H, W


def label_components(labels: torch.Tensor, connectivity: int, root: torch.Tensor, ids: torch.Tensor, count: torch.Tensor,
                     workspace: torch.Tensor) -> None:
    """Connected components of a batch of label maps (include/cclip_hip.h, cclip_label_components): labels uint8 [B, H, W], 255 =
    none, joined over 4- or 8-neighbours of equal label inside one image -> root int32 [B, H, W] (the flat index of the
    component's first pixel, -1 for none), ids int32 [B, H, W] (0 .. n - 1 in ascending order of root, -1 for none), count int32
    [1] (n, left on the device).  workspace: int32, at least ceil(B H W / COMPONENTS_GROUP) elements.  Contiguous cuda tensors
    on one device; no CPU path.  Two calls give equal bytes."""
    fname = "label_components"
    B, H, W = _component_maps(fname, labels, [(root, "root", torch.int32), (ids, "ids", torch.int32)])
    _cuda_operands(fname, [(labels, "labels", torch.uint8), (count, "count", torch.int32), (workspace, "workspace", torch.int32)], labels)
    if connectivity not in (4, 8):
        raise ValueError(f"{fname}: connectivity must be 4 or 8, got {connectivity!r}")
    if count.numel() != 1:
        raise ValueError(f"{fname}: count must hold one element, got {tuple(count.shape)}")
    need = (B * H * W + COMPONENTS_GROUP - 1) // COMPONENTS_GROUP
    if workspace.numel() < need:
        raise ValueError(f"{fname}: workspace must hold at least {need} int32 elements, got {workspace.numel()}")
    check(lib.cclip_label_components(_p(labels), c_int(B), c_int(H), c_int(W), c_int(int(connectivity)), _p(root), _p(ids), _p(count),
                                     _p(workspace), c_long(workspace.numel()), _stream()), "cclip_label_components")


def component_stats(labels: torch.Tensor, root: torch.Tensor, ids: torch.Tensor, n: int, label: torch.Tensor, image: torch.Tensor,
                    first: torch.Tensor, area: torch.Tensor, box: torch.Tensor, *, conf: Optional[torch.Tensor] = None,
                    qsum: Optional[torch.Tensor] = None) -> None:
    """Per-component statistics of a labelling (include/cclip_hip.h, cclip_component_stats): labels uint8, root / ids int32
    [B, H, W] as label_components left them and n = its count, read by the caller -> label uint8 [n], image, first, area int32
    [n], box int32 [n, 4] (x0, y0, x1, y1; half-open, image coordinates) and, with conf fp32 [B, H, W], qsum int64 [n]: the sum of
    the 16.16 fixed-point confidences (never negative: at most 2^44).  n = 0 launches nothing.  Contiguous cuda tensors on one
    device; no CPU path.  Two calls give equal bytes."""
    fname = "component_stats"
    B, H, W = _component_maps(fname, labels, [(root, "root", torch.int32), (ids, "ids", torch.int32), (conf, "conf", torch.float32)])
    outs = [(label, "label", torch.uint8), (image, "image", torch.int32), (first, "first", torch.int32), (area, "area", torch.int32),
            (box, "box", torch.int32)]
    if qsum is not None:
        outs.append((qsum, "qsum", torch.int64))
    _cuda_operands(fname, [(labels, "labels", torch.uint8)] + outs, labels)
    if (conf is None) != (qsum is None):
        raise ValueError(f"{fname}: conf and qsum go together; give both or neither")
    if int(n) != n or not 0 <= n <= B * H * W:
        raise ValueError(f"{fname}: n must be an integer in [0, {B * H * W}], got {n!r}")
    n = int(n)
    for t, name, _ in outs:
        want = (n, 4) if name == "box" else (n,)
        if tuple(t.shape) != want:
            raise ValueError(f"{fname}: {name} must be {list(want)}, got {tuple(t.shape)}")
    if n == 0:
        return
    check(lib.cclip_component_stats(_p(labels), _p(conf), _p(root), _p(ids), c_int(B), c_int(H), c_int(W), c_int(n), _p(label),
                                    _p(image), _p(first), _p(area), _p(box), _p(qsum), _stream()), "cclip_component_stats")


AGREEMENT_MAX_BAND = 32
AGREEMENT_HIST_CELLS = 2048     # confusion cells a tile gathers in LDS: n_classes (n_classes + 1) above it takes the wave-combine path


def label_agreement(pred: torch.Tensor, gt: torch.Tensor, n_classes: int, band: int, confusion: torch.Tensor, bad: torch.Tensor,
                    bands: Optional[torch.Tensor] = None, per_image: bool = False, accumulate: bool = False) -> None:
    """The integer counts behind mean IoU and boundary IoU (include/cclip_hip.h, cclip_label_agreement): pred, gt uint8 [B, H, W]
    -> confusion int64 [R, C, C + 1] (gt class by pred class, "none" = 255 in the last column; gt == 255 is ignored), bad int64
    [R, 2] (labels in [C, 254] in gt / in pred) and, with band = d > 0, bands int64 [R, C, 3] = (|G_c|, |P_c|, |G_c n P_c|) of the
    band of half-width d (None when band == 0).  R = B with per_image, else 1.  accumulate adds to what the outputs hold.
    Contiguous cuda tensors on one device; no CPU path.  Two calls give equal bytes."""
    fname = "label_agreement"
    _cuda_operands(fname, [(pred, "pred", torch.uint8), (gt, "gt", torch.uint8)], pred)
    if pred.dim() != 3 or min(pred.shape) < 1:
        raise ValueError(f"{fname}: pred must be [B, H, W] with no empty dimension, got {tuple(pred.shape)}")
    B, H, W = pred.shape
    if tuple(gt.shape) != (B, H, W):
        raise ValueError(f"{fname}: gt must be {[B, H, W]}, got {tuple(gt.shape)}")
    if H > OVERLAY_MAX_SIDE or W > OVERLAY_MAX_SIDE:
        raise ValueError(f"{fname}: height {H}, width {W}: each must lie in [1, {OVERLAY_MAX_SIDE}]")
    if B * H * W > _INT32_MAX:
        raise ValueError(f"{fname}: pred holds {B * H * W} pixels; at most 2^31 - 1")
    if isinstance(n_classes, bool) or int(n_classes) != n_classes or not 1 <= n_classes <= DENSE_MAX_CLASSES:
        raise ValueError(f"{fname}: n_classes must be an integer in [1, {DENSE_MAX_CLASSES}] (label 255 means none), got {n_classes!r}")
    if isinstance(band, bool) or int(band) != band or not 0 <= band <= AGREEMENT_MAX_BAND:
        raise ValueError(f"{fname}: band must be an integer in [0, {AGREEMENT_MAX_BAND}], got {band!r}")
    C, d, R = int(n_classes), int(band), (B if per_image else 1)
    if (d > 0) != (bands is not None):
        raise ValueError(f"{fname}: bands goes with band > 0; got band {d} and bands {'given' if bands is not None else 'missing'}")
    outs = [(confusion, "confusion", (R, C, C + 1)), (bad, "bad", (R, 2))] + ([(bands, "bands", (R, C, 3))] if bands is not None else [])
    _cuda_operands(fname, [(pred, "pred", torch.uint8)] + [(t, name, torch.int64) for t, name, _ in outs], pred)
    for t, name, want in outs:
        if tuple(t.shape) != want:
            raise ValueError(f"{fname}: {name} must be {list(want)}, got {tuple(t.shape)}")
        if t.data_ptr() % 8:
            raise ValueError(f"{fname}: {name} must start on an 8-byte boundary")
    check(lib.cclip_label_agreement(_p(pred), _p(gt), c_int(B), c_int(H), c_int(W), c_int(C), c_int(d), c_int(int(bool(per_image))),
                                    c_int(int(bool(accumulate))), _p(confusion), _p(bad), _p(bands), _stream()), "cclip_label_agreement")


PROTOTYPES_SLAB = 64            # cells of one partial sum: the split of the K g g cells is a function of K and g alone


def dense_prototypes_workspace(K: int, grid: int, n_classes: int, embed_dim: int) -> int:
    """Bytes of scratch ops.dense_prototypes needs (the header's closed form, restated): per slab of PROTOTYPES_SLAB cells and per
    class, embed_dim partial sums, one weight and one patch count."""
    return -(-(K * grid * grid) // PROTOTYPES_SLAB) * n_classes * (embed_dim + 2) * 4


def dense_prototypes(feat: torch.Tensor, masks: torch.Tensor, boxes: torch.Tensor, grid: int, n_classes: int, min_share8: int,
                     sums: torch.Tensor, weight: torch.Tensor, patches: torch.Tensor, pixels: torch.Tensor, bad: torch.Tensor, *,
                     image: Optional[torch.Tensor] = None, accumulate: bool = False, workspace: Optional[torch.Tensor] = None) -> None:
    """Masked average pooling of per-patch features into class prototypes (include/cclip_hip.h, cclip_dense_prototypes): feat fp32
    [K * grid * grid, E] (rows may be strided; encode_image_dense viewed flat), masks uint8 [B, H, W] (class index < n_classes,
    255 = ignore), boxes int32 [K, 4] = (x0, y0, x1, y1) of window k in picture image[k] (int32 [K]; None: picture 0) -> sums fp32
    [C, E] = sum of w * unit feature over the cells whose share of class c is at least min_share8 / 256 (w = that share), weight
    fp32 [C], patches int64 [C], pixels int64 [C] and bad int64 [1] (mask values in [C, 254]).  accumulate adds to what the outputs
    hold.  The boxes are NOT read back: an empty, inverted or oversized box or an image index outside [0, B) contributes nothing.
    workspace: 16-byte aligned uint8 / fp32 scratch of dense_prototypes_workspace(K, grid, C, E) bytes, allocated when None.
    cuda tensors on one device; no CPU path.  Two calls give equal bytes."""
    fname = "dense_prototypes"
    tensors = [(feat, "feat", torch.float32), (masks, "masks", torch.uint8), (boxes, "boxes", torch.int32), (sums, "sums", torch.float32),
               (weight, "weight", torch.float32), (patches, "patches", torch.int64), (pixels, "pixels", torch.int64), (bad, "bad", torch.int64)]
    if image is not None:
        tensors.append((image, "image", torch.int32))
    _cuda_operands(fname, tensors, feat, strided=("feat",))
    if isinstance(grid, bool) or int(grid) != grid or not 1 <= grid <= OVERLAY_MAX_SIDE:
        raise ValueError(f"{fname}: grid must be an integer in [1, {OVERLAY_MAX_SIDE}], got {grid!r}")
    if isinstance(n_classes, bool) or int(n_classes) != n_classes or not 1 <= n_classes <= DENSE_MAX_CLASSES:
        raise ValueError(f"{fname}: n_classes must be an integer in [1, {DENSE_MAX_CLASSES}] (label 255 means ignore), got {n_classes!r}")
    if isinstance(min_share8, bool) or int(min_share8) != min_share8 or not 0 <= min_share8 <= 256:
        raise ValueError(f"{fname}: min_share8 must be an integer in [0, 256], got {min_share8!r}")
    g, C = int(grid), int(n_classes)
    M, E = feat.shape
    if E < 4 or E % 4 or E > DENSE_MAX_EMBED:
        raise ValueError(f"{fname}: feat has embedding width {E}; it must be a multiple of 4 in [4, {DENSE_MAX_EMBED}]")
    if M < 1 or M % (g * g) or M // (g * g) > DENSE_MAX_WINDOWS:
        raise ValueError(f"{fname}: feat has {M} rows; it must hold between 1 and {DENSE_MAX_WINDOWS} windows of grid * grid = {g * g} rows")
    K = M // (g * g)
    if M > 1 and (feat.stride(0) < E or feat.stride(0) % 4):
        raise ValueError(f"{fname}: feat must have a row stride >= {E} that is a multiple of 4, got {feat.stride(0)}")
    if feat.data_ptr() % 16:
        raise ValueError(f"{fname}: feat must start on a 16-byte boundary")
    if masks.dim() != 3 or min(masks.shape) < 1:
        raise ValueError(f"{fname}: masks must be [B, H, W] with no empty dimension, got {tuple(masks.shape)}")
    B, H, W = masks.shape
    if H > OVERLAY_MAX_SIDE or W > OVERLAY_MAX_SIDE:
        raise ValueError(f"{fname}: height {H}, width {W}: each must lie in [1, {OVERLAY_MAX_SIDE}]")
    if B * H * W > _INT32_MAX:
        raise ValueError(f"{fname}: masks holds {B * H * W} pixels; at most 2^31 - 1")
    if tuple(boxes.shape) != (K, 4):
        raise ValueError(f"{fname}: boxes must be [{K}, 4] as (x0, y0, x1, y1), got {tuple(boxes.shape)}")
    if image is not None and tuple(image.shape) != (K,):
        raise ValueError(f"{fname}: image must be [{K}], got {tuple(image.shape)}")
    for t, name, want, align in ((sums, "sums", (C, E), 4), (weight, "weight", (C,), 4), (patches, "patches", (C,), 8),
                                 (pixels, "pixels", (C,), 8), (bad, "bad", (1,), 8)):
        if tuple(t.shape) != want:
            raise ValueError(f"{fname}: {name} must be {list(want)}, got {tuple(t.shape)}")
        if t.data_ptr() % align:
            raise ValueError(f"{fname}: {name} must start on a {align}-byte boundary")
    need = dense_prototypes_workspace(K, g, C, E)
    if workspace is None:
        workspace = torch.empty(need, device=feat.device, dtype=torch.uint8)
    else:
        if not isinstance(workspace, torch.Tensor) or workspace.device != feat.device or not workspace.is_contiguous():
            raise ValueError(f"{fname}: workspace must be a contiguous cuda tensor on {feat.device}, got {getattr(workspace, 'device', type(workspace))}")
        if workspace.dtype not in (torch.uint8, torch.float32) or workspace.numel() * workspace.element_size() < need or workspace.data_ptr() % 16:
            raise ValueError(f"{fname}: workspace must be a uint8 or float32 tensor of at least {need} bytes on a 16-byte boundary, got "
                             f"{workspace.dtype}, {workspace.numel() * workspace.element_size()} bytes, address % 16 = {workspace.data_ptr() % 16}")
    ldf = feat.stride(0) if M > 1 else E
    check(lib.cclip_dense_prototypes(_p(feat), c_long(ldf), _p(masks), _p(boxes), _p(image), c_int(K), c_int(g), c_int(C), c_int(E),
                                     c_int(B), c_int(H), c_int(W), c_int(int(min_share8)), c_int(int(bool(accumulate))), _p(sums),
                                     _p(weight), _p(patches), _p(pixels), _p(bad), _p(workspace),
                                     c_long(workspace.numel() * workspace.element_size()), _stream()), "cclip_dense_prototypes")


# --------------------------------------------------------------------------------------------
# fp8 (e4m3) inference projections
# --------------------------------------------------------------------------------------------
def quantize_rows_fp8(x16: torch.Tensor, out8: torch.Tensor, scale: torch.Tensor) -> None:
    """x16 [R, C] 16-bit -> out8 [R, C] uint8 (e4m3 bytes), scale [R] fp32 (x ~= scale[r] * fp8)."""
    _req16(x16, "x16"); _req(scale, torch.float32, "scale")
    assert out8.dtype == torch.uint8 and x16.dim() == 2 and out8.shape == x16.shape and x16.stride(1) == 1 and out8.stride(1) == 1
    R, C = x16.shape
    check(_fn("cclip_quantize_rows_fp8", x16)(_p(x16), c_long(x16.stride(0)), c_int(R), c_int(C), _p(out8), c_long(out8.stride(0)),
                                             _p(scale), _stream()), "cclip_quantize_rows_fp8")


def layernorm_fwd_fp8(x: torch.Tensor, gamma, beta, out8: torch.Tensor, scale: torch.Tensor, *, rows: int, eps: float = 1e-5) -> None:
    _req(x, torch.float32, "x"); _req(scale, torch.float32, "scale")
    assert out8.dtype == torch.uint8 and out8.stride(-1) == 1
    check(lib.cclip_layernorm_fwd_fp8(_p(x), c_long(x.stride(-2)), c_int(rows), c_int(x.shape[-1]), _p(gamma), _p(beta), c_float(eps),
                                      _p(out8), c_long(out8.stride(-2)), _p(scale), _stream()), "cclip_layernorm_fwd_fp8")


def quantize_mx_fp8(x16: torch.Tensor, out8: torch.Tensor, block_scale: torch.Tensor, *, rows: Optional[int] = None) -> None:
    """x16 [R, C] 16-bit (C % 32 == 0) -> out8 [R, C] uint8 (e4m3 bytes) + block_scale [ceil(C/128), R, 4] uint8 (E8M0): every
    32 consecutive columns of a row share the power-of-two scale 2^(e - 127) (the block-scaled MFMA's operand format); the
    scale of (row r, block b) is block_scale[b >> 2, r, b & 3] (K-tile major: what the consuming GEMM reads per K-tile is
    contiguous)."""
    _req16(x16, "x16")
    assert out8.dtype == torch.uint8 and x16.dim() == 2 and out8.shape[1] == x16.shape[1] and x16.stride(1) == 1 and out8.stride(1) == 1
    R, C = x16.shape
    R = R if rows is None else rows
    _req_mx(block_scale, R, C, "block_scale")
    check(_fn("cclip_quantize_mx_fp8", x16)(_p(x16), c_long(x16.stride(0)), c_int(R), c_int(C), _p(out8), c_long(out8.stride(0)),
                                           _p(block_scale), c_long(block_scale.stride(0)), _stream()), "cclip_quantize_mx_fp8")


def _req_mx(t: torch.Tensor, rows: int, cols: int, name: str):
    if not (t.dtype == torch.uint8 and t.is_cuda and t.dim() == 3 and t.shape[0] * 128 >= cols and t.shape[1] >= rows and t.shape[2] == 4
            and t.stride(2) == 1 and t.stride(1) == 4):
        raise TypeError(f"{name}: expected a cuda uint8 [>= {(cols + 127) // 128}, >= {rows}, 4] block-scale tensor, got {tuple(t.shape)} {t.dtype}")


def mx_scale_buffer(rows: int, cols: int, device) -> torch.Tensor:
    """Block-scale tensor for a [rows, cols] block-scaled e4m3 operand: uint8 [ceil(cols/128), rows, 4]."""
    return torch.empty((cols + 127) // 128, rows, 4, device=device, dtype=torch.uint8)


class Fp8GemmDesc(ctypes.Structure):
    """include/cclip_hip.h: cclip_fp8_gemm_desc"""
    _fields_ = [("A", c_void_p), ("lda", c_long), ("scale_a", c_void_p), ("block_scale_a", c_void_p), ("ld_block_scale_a", c_long),
                ("B", c_void_p), ("ldb", c_long), ("scale_b", c_void_p), ("M", c_int), ("N", c_int), ("K", c_int),
                ("bias", c_void_p), ("act", c_int), ("out16", c_void_p), ("ldc", c_long),
                ("out_fp8", c_void_p), ("ld_out_fp8", c_long), ("out_block_scale", c_void_p), ("ld_out_block_scale", c_long),
                ("out_f32", c_void_p), ("residual", c_void_p), ("ldf", c_long)]


def gemm_fp8(A8, scale_a, B8, scale_b, out16=None, *, bias=None, act: int = ACT_NONE, M: Optional[int] = None,
             block_scale_a=None, out_mx=None, out_f32=None, residual=None, half=None) -> None:
    """act(sa[m] * sb[n] * sum_k A8[m][k] B8[n][k] + bias[n]); A8 [M,K], B8 [N,K] uint8 e4m3, sb per output channel.
    A's scale: scale_a [M] fp32 per row, or block_scale_a [K/128, M, 4] uint8 E8M0 per 32-deep k block (applied by the MFMA).
    Output (exactly one): out16 (16-bit) | out_mx = (out8 [M,N] uint8, block_scale [N/128, M, 4] uint8): e4m3 + E8M0 per 32 columns,
    the next GEMM's block-scaled A operand | out_f32 (+ residual, fp32, may alias): the residual stream.
    `half`: torch.bfloat16 / torch.float16 picks the library twin when no 16-bit tensor is among the arguments."""
    assert A8.dtype == torch.uint8 and B8.dtype == torch.uint8 and A8.stride(1) == 1 and B8.stride(1) == 1
    Mx, K = A8.shape
    N = B8.shape[0]
    M = Mx if M is None else M
    assert B8.shape[1] == K
    d = Fp8GemmDesc()
    d.A, d.lda, d.B, d.ldb, d.scale_b = A8.data_ptr(), A8.stride(0), B8.data_ptr(), B8.stride(0), scale_b.data_ptr()
    d.M, d.N, d.K, d.act = M, N, K, act
    d.bias = 0 if bias is None else bias.data_ptr()
    if block_scale_a is not None:
        _req_mx(block_scale_a, M, K, "block_scale_a")
        d.block_scale_a, d.ld_block_scale_a = block_scale_a.data_ptr(), block_scale_a.stride(0)
    else:
        _req(scale_a, torch.float32, "scale_a")
        d.scale_a = scale_a.data_ptr()
    if out16 is not None:
        _req16(out16, "out16")
        assert out16.shape[1] == N and out16.shape[0] >= M
        d.out16, d.ldc = out16.data_ptr(), out16.stride(0)
    if out_mx is not None:
        o8, omx = out_mx
        assert o8.dtype == torch.uint8 and o8.shape[1] == N and o8.shape[0] >= M and o8.stride(1) == 1
        _req_mx(omx, M, N, "out_mx[1]")
        d.out_fp8, d.ld_out_fp8, d.out_block_scale, d.ld_out_block_scale = o8.data_ptr(), o8.stride(0), omx.data_ptr(), omx.stride(0)
    if out_f32 is not None:
        _req(out_f32, torch.float32, "out_f32"); _req(residual, torch.float32, "residual")
        assert out_f32.shape[1] == N and out_f32.stride(0) == residual.stride(0)
        d.out_f32, d.residual, d.ldf = out_f32.data_ptr(), residual.data_ptr(), out_f32.stride(0)
    ev = None
    if GEMM_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    f16 = (out16.dtype if out16 is not None else half) == torch.float16
    fn = lib.cclip_gemm_fp8_ex_f16 if f16 else lib.cclip_gemm_fp8_ex
    check(fn(ctypes.byref(d), _stream()), "cclip_gemm_fp8_ex")
    if ev is not None:
        ev[1].record()
        GEMM_EVENTS.append((ev[0], ev[1], 2.0 * M * N * K, (1, 1), (M, N, K)))


class BlockPtrs(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("ln1_w", "ln1_b", "w_qkv", "b_qkv", "w_o", "b_o", "ln2_w", "ln2_b", "w_fc", "b_fc", "w_proj", "b_proj")]


class DecodeDesc(ctypes.Structure):
    _fields_ = [("n_layer", c_int), ("n_seq", c_int), ("width", c_int), ("heads", c_int), ("hidden", c_int), ("act", c_int),
                ("linear_layout", c_int), ("pos", c_int),
                ("blocks", ctypes.POINTER(BlockPtrs)), ("x", c_void_p), ("kcache", c_void_p), ("vcache", c_void_p),
                ("ld_layer", c_long), ("ld_seq", c_long), ("scratch16", c_void_p),
                ("lnf_w", c_void_p), ("lnf_b", c_void_p), ("wte16", c_void_p), ("vocab", c_int), ("logits", c_void_p), ("ld_logits", c_long)]


def block_ptr_array(blocks):
    """ctypes array of per-layer weight pointers for cclip_gpt2_decode_step (blocks: cclip_hip.stack.BlockWeights)."""
    arr = (BlockPtrs * len(blocks))()
    for i, w in enumerate(blocks):
        for n, _ in BlockPtrs._fields_:
            t = getattr(w, n)
            setattr(arr[i], n, 0 if t is None else t.data_ptr())
    return arr


def decode_step_desc(blocks_arr, n_layer, x, kcache, vcache, pos, scratch16, *, heads, hidden, act, linear_layout,
                     lnf_w=None, lnf_b=None, wte16=None, logits=None, into: Optional[DecodeDesc] = None) -> DecodeDesc:
    """The DecodeDesc (a new one, or `into`) of one step for the x.shape[0] sequences of x (fp32 [n_seq, width]), with the checks
    of the layout the kernels index by: cache rows dense and `width` apart, k and v strided alike, a scratch of
    n_seq * (5 * width + hidden) cache-dtype elements.  Reads shapes, strides and addresses only: no library, no GPU."""
    s = DecodeDesc() if into is None else into
    nb, D = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and x.device == kcache.device
    assert kcache.dim() == 4 and kcache.stride(3) == 1 and kcache.stride(2) == D and kcache.stride() == vcache.stride()
    assert scratch16.numel() >= nb * (5 * D + hidden) and scratch16.dtype == kcache.dtype
    s.n_layer, s.n_seq, s.width, s.heads, s.hidden, s.act, s.linear_layout, s.pos = n_layer, nb, D, heads, hidden, act, int(linear_layout), pos
    s.blocks = blocks_arr
    s.x, s.kcache, s.vcache = x.data_ptr(), kcache.data_ptr(), vcache.data_ptr()
    s.ld_layer, s.ld_seq = kcache.stride(0), kcache.stride(1)
    s.scratch16 = scratch16.data_ptr()
    if wte16 is not None:
        s.lnf_w, s.lnf_b, s.wte16, s.vocab = lnf_w.data_ptr(), lnf_b.data_ptr(), wte16.data_ptr(), wte16.shape[0]
    if logits is not None:
        assert logits.dtype == torch.float32 and logits.device == kcache.device
        s.logits, s.ld_logits = logits.data_ptr(), logits.stride(0)
    return s


def _launch(name: str, d, kcache) -> None:
    _req16(kcache, "kcache")
    check(_fn(name, kcache)(ctypes.byref(d), _stream()), name)


def gpt2_decode_step(blocks_arr, n_layer, x, kcache, *args, **kw) -> None:
    """One KV-cached decode step for x.shape[0] sequences, issued natively (cclip_gpt2_decode_step; arguments: decode_step_desc).
    kcache / vcache: [n_layer, n_seq_alloc, max_len, width] 16-bit; x: fp32 [n_seq, width] (in place)."""
    _launch("cclip_gpt2_decode_step", decode_step_desc(blocks_arr, n_layer, x, kcache, *args, **kw), kcache)


class BeamDesc(ctypes.Structure):
    _fields_ = [("step", DecodeDesc),
                ("n_steps", c_int), ("first", c_int), ("stop_token", c_int), ("ld_tokens", c_int), ("max_len", c_int), ("grid_cap", c_int),
                ("temperature", c_float),
                ("first_logits", c_void_p), ("wte_f32", c_void_p), ("wpe_f32", c_void_p),
                ("slot_of", c_void_p), ("tokens", c_void_p),
                ("scores", c_void_p), ("seq_lengths", c_void_p), ("is_stopped", c_void_p),
                ("state", c_void_p), ("select_ws", c_void_p)]


class BeamBatchDesc(ctypes.Structure):
    _fields_ = [("step", DecodeDesc),
                ("n_cap", c_int), ("beams", c_int), ("n_steps", c_int), ("stop_token", c_int), ("ld_tokens", c_int), ("max_len", c_int),
                ("grid_cap", c_int), ("temperature", c_float),
                ("first_logits", c_void_p), ("wte_f32", c_void_p), ("wpe_f32", c_void_p),
                ("slot_of", c_void_p), ("tokens", c_void_p),
                ("scores", c_void_p), ("seq_lengths", c_void_p), ("is_stopped", c_void_p),
                ("state", c_void_p), ("cap_state", c_void_p), ("select_ws", c_void_p)]


BEAM_MAX_BEAMS, BEAM_MAX_LAYERS, BEAM_SELECT_WS_FLOATS = 8, 24, 256 * 8 * 20
BEAM_BATCH_MAX_ROWS = 64
_BEAM_BUFFERS = ("slot_of", "tokens", "scores", "seq_lengths", "is_stopped", "state", "select_ws")


def _alloc_beam_state(st, n_cap: int, n_beams: int, max_len: int, max_tokens: int, device) -> None:
    """The buffers both persistent kernels keep per search: row c * n_beams + b is beam b of caption c."""
    R = n_cap * n_beams
    st.n_beams, st.max_len = n_beams, max_len
    st.tokens = torch.zeros(R, max_tokens, device=device, dtype=torch.int32)
    st.scores = torch.zeros(R, device=device, dtype=torch.float32)
    st.seq_lengths = torch.ones(R, device=device, dtype=torch.float32)
    st.is_stopped = torch.zeros(R, device=device, dtype=torch.int32)
    st.state = torch.zeros(8, device=device, dtype=torch.int32)
    st.select_ws = torch.empty(n_cap * BEAM_SELECT_WS_FLOATS, device=device, dtype=torch.float32)
    st.x = None                    # fp32 [R, width]: the first descriptor filled from this state allocates it


class BeamState:
    """Device state of one persistent beam search (cclip_gpt2_beam_search): token rows, scores, lengths, stop flags, the
    cache-slot table and the kernel's bookkeeping words."""

    def __init__(self, n_beams: int, max_len: int, max_tokens: int, device):
        assert 1 <= n_beams <= BEAM_MAX_BEAMS
        _alloc_beam_state(self, 1, n_beams, max_len, max_tokens, device)
        self.slot_of = torch.zeros(max_len, BEAM_MAX_BEAMS, device=device, dtype=torch.int32)


class BeamBatchState:
    """Device state of one batched persistent beam search (cclip_gpt2_beam_search_batch) over n_cap captions: BeamState's
    buffers for the n_cap * beams rows, the per-caption cache-slot tables and the per-caption bookkeeping words."""

    def __init__(self, n_cap: int, n_beams: int, max_len: int, max_tokens: int, device):
        assert n_beams >= 1 and n_cap >= 1                 # (> 8 beams or > 64 rows: the kernel refuses them)
        _alloc_beam_state(self, n_cap, n_beams, max_len, max_tokens, device)
        self.n_cap = n_cap
        self.slot_of = torch.zeros(n_cap, max_len, BEAM_MAX_BEAMS, device=device, dtype=torch.int32)
        self.cap_state = torch.zeros(n_cap, 8, device=device, dtype=torch.int32)


def _fill_beam_desc(d, blocks_arr, n_layer, st, kcache, vcache, pos, scratch16, n_steps, *, wte16, wte_f32, wpe_f32, temperature,
                    stop_token, first_logits=None, grid_cap: int = 0, linear_layout: bool = False, **step_kw) -> None:
    """What BeamDesc and BeamBatchDesc share: `step` for the st.tokens.shape[0] rows of the search (step_kw: heads, hidden, act,
    lnf_w, lnf_b and, one caption only, logits), the beam-only checks, and the state object's buffers and the search scalars,
    which the two structs name alike."""
    rows, (V, D) = st.tokens.shape[0], wte16.shape
    if st.x is None:
        st.x = torch.empty(rows, D, device=kcache.device, dtype=torch.float32)
    decode_step_desc(blocks_arr, n_layer, st.x, kcache, vcache, pos, scratch16, wte16=wte16, linear_layout=linear_layout, into=d.step,
                     **step_kw)
    assert n_layer <= BEAM_MAX_LAYERS and kcache.shape[1] == rows and kcache.shape[2] == st.max_len
    assert wte_f32.dtype == torch.float32 and wpe_f32.dtype == torch.float32
    assert wte_f32.is_contiguous() and wpe_f32.is_contiguous() and wte16.is_contiguous() and wpe_f32.shape[0] >= st.max_len
    d.n_steps, d.stop_token, d.ld_tokens, d.max_len, d.grid_cap = n_steps, stop_token, st.tokens.stride(0), st.max_len, grid_cap
    d.temperature = temperature
    d.wte_f32, d.wpe_f32 = wte_f32.data_ptr(), wpe_f32.data_ptr()
    if first_logits is not None:                              # one row of V per caption
        assert first_logits.dtype == torch.float32 and first_logits.device == kcache.device
        assert first_logits.is_contiguous() and first_logits.numel() == rows // st.n_beams * V
        d.first_logits = first_logits.data_ptr()
    for name in _BEAM_BUFFERS:
        setattr(d, name, getattr(st, name).data_ptr())


def beam_search_desc(*args, first_logits=None, **kw) -> BeamDesc:
    """BeamDesc of a one-caption search (arguments: _fill_beam_desc, st a BeamState).  first_logits ([vocab] fp32, the prefill's
    last row) given: the launch starts with the one-sequence selection of the first loop iteration.  The cache ([n_layer,
    n_beams, max_len, width]) holds the prefix in slot 0; beams are reordered through st.slot_of."""
    d = BeamDesc()
    _fill_beam_desc(d, *args, first_logits=first_logits, **kw)
    d.first = int(first_logits is not None)
    return d


def gpt2_beam_search(blocks_arr, n_layer, st: BeamState, kcache, *args, **kw) -> None:
    """`n_steps` KV-cached decode steps + beam selections in ONE persistent launch (cclip_gpt2_beam_search; Conv1D layout;
    arguments: beam_search_desc)."""
    _launch("cclip_gpt2_beam_search", beam_search_desc(blocks_arr, n_layer, st, kcache, *args, **kw), kcache)


def beam_search_batch_desc(blocks_arr, n_layer, st: BeamBatchState, kcache, vcache, pos, scratch16, n_steps, *, first_logits, **kw) -> BeamBatchDesc:
    """BeamBatchDesc of a search over st.n_cap captions (arguments: _fill_beam_desc).  first_logits: [n_cap, vocab] fp32, the
    prefills' last rows; kcache / vcache: [n_layer, n_cap * beams, max_len, width], caption c's prefix in slot c * beams."""
    assert first_logits.dim() == 2 and first_logits.shape[0] == st.n_cap and st.tokens.shape[1] >= n_steps + 1
    d = BeamBatchDesc()
    _fill_beam_desc(d, blocks_arr, n_layer, st, kcache, vcache, pos, scratch16, n_steps, first_logits=first_logits, **kw)
    d.n_cap, d.beams, d.cap_state = st.n_cap, st.n_beams, st.cap_state.data_ptr()
    return d


def gpt2_beam_search_batch(blocks_arr, n_layer, st: BeamBatchState, kcache, *args, **kw) -> None:
    """The first selection of every caption, then up to `n_steps` KV-cached decode steps + selections of all st.n_cap captions
    in ONE persistent launch (cclip_gpt2_beam_search_batch; Conv1D layout; arguments: beam_search_batch_desc).  Raises on a
    shape the kernel refuses (> 64 rows, > 8 beams, nn.Linear layout)."""
    _launch("cclip_gpt2_beam_search_batch", beam_search_batch_desc(blocks_arr, n_layer, st, kcache, *args, **kw), kcache)


# --------------------------------------------------------------------------------------------
# exact fp32 GEMM:  C = alpha * A @ B^T-like contraction with arbitrary strides
# --------------------------------------------------------------------------------------------
def gemm_f32(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, *, alpha: float = 1.0, beta: float = 0.0,
             alpha_log_dev: Optional[torch.Tensor] = None) -> None:
    """C[m,n] = alpha * sum_k A[m,k] * B[n,k] + beta*C.  A: [M,K], B: [N,K] as (possibly transposed) 2-D views."""
    _req(A, torch.float32, "A"); _req(B, torch.float32, "B"); _req(C, torch.float32, "C")
    M, K = A.shape
    N, Kb = B.shape
    assert K == Kb and C.shape == (M, N) and C.stride(1) == 1
    check(lib.cclip_gemm_f32(_p(A), c_long(A.stride(0)), c_long(A.stride(1)), _p(B), c_long(B.stride(0)),
                             c_long(B.stride(1)), c_int(M), c_int(N), c_int(K), c_float(alpha), _p(alpha_log_dev), c_float(beta), _p(C),
                             c_long(C.stride(0)), _stream()), "cclip_gemm_f32")


# --------------------------------------------------------------------------------------------
# embeddings
# --------------------------------------------------------------------------------------------
def patchify(image: torch.Tensor, out_bf16: torch.Tensor, P: int) -> None:
    _req(image, torch.float32, "image")
    assert image.is_contiguous() and image.dim() == 4 and image.shape[1] == 3 and image.shape[2] == image.shape[3]
    check(_fn("cclip_patchify", out_bf16)(_p(image), _p(out_bf16), c_int(image.shape[0]), c_int(image.shape[2]), c_int(P), _stream()),
          "cclip_patchify")


def vit_embed_ln(patch_out, cls, pos, gamma, beta, x, *, rows: int, T: int, x0=None, mean=None, rstd=None, eps=1e-5):
    D = patch_out.shape[-1]
    check(lib.cclip_vit_embed_ln(_p(patch_out), _p(cls), _p(pos), c_int(rows), c_int(T), c_int(D), _p(gamma), _p(beta),
                                 c_float(eps), _p(x0), _p(x), _p(mean), _p(rstd), _stream()), "cclip_vit_embed_ln")


def text_embed(text_i32, emb, pos, x, *, rows: int, L: int) -> None:
    _req(text_i32, torch.int32, "text")
    check(lib.cclip_text_embed(_p(text_i32), _p(emb), _p(pos), c_int(rows), c_int(L), c_int(emb.shape[1]),
                               c_int(emb.shape[0]), _p(x), _stream()), "cclip_text_embed")


SCATTER_DETERMINISTIC = True     # False: the one-launch fp32-atomics kernel (sums rows of one token id in hardware order)
_SEG_CHUNK = 64


def embed_scatter_tables(text_i32, V: int, *, rows: int, keep: Optional[torch.Tensor] = None):
    """Index tables of the deterministic embedding-gradient sum (see embed_scatter_add): the row list sorted by token id
    (stable) and, per sorted position, the chunk / run bookkeeping csrc/embed.hip walks.  Integer math on a [rows] vector that
    depends on the token ids only - a training step can build it while the forward pass runs (clip/model.py does, on a side
    stream).  The sort is the device library's; the tables come from one scan-free kernel (cclip_embed_tables: two binary
    searches per position; round 2 built them from ~25 small torch launches incl. three single-block scans, 0.6 ms)."""
    tok = text_i32[:rows].clamp(0, V - 1)
    if keep is not None:                                  # dropped rows sort to the end under a sentinel id and form no chunk
        tok = torch.where(keep[:rows], tok, torch.full_like(tok, V))
    st, perm = torch.sort(tok.to(torch.int32), stable=True)
    order = perm.to(torch.int32)
    tabs = torch.empty((3, rows), device=text_i32.device, dtype=torch.int32)
    check(lib.cclip_embed_tables(_p(st), c_int(rows), c_int(V), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _stream()), "cclip_embed_tables")
    return (order, st, tabs[0], tabs[1], tabs[2])


def embed_scatter_add(text_i32, dx, demb, *, rows: int, L: Optional[int] = None, seq_stride: Optional[int] = None,
                      seq_off: int = 0, keep: Optional[torch.Tensor] = None, tables=None, scratch=None) -> None:
    """demb[text[r]] += dx[(r // L) * seq_stride + seq_off + r % L] for r < rows (the embedding-table gradient).
    keep: optional bool [rows] - rows known to carry a zero gradient (text positions after EOT) can be dropped up front.
    tables: embed_scatter_tables(text_i32, V, rows=rows, keep=keep) built earlier (same text / keep).

    Deterministic by default: the row list is sorted by token id (stable) and every run of equal ids is summed in list order
    by the wave that owns its embedding row, runs longer than 64 rows through ordered partials (csrc/embed.hip).  The sort /
    run bookkeeping is integer index math on a [rows] vector; every float is added by the HIP kernels."""
    L = rows if L is None else L
    seq_stride = L if seq_stride is None else seq_stride
    if not SCATTER_DETERMINISTIC:
        check(lib.cclip_embed_scatter_add(_p(text_i32), _p(dx), c_long(dx.stride(-2)), c_int(rows), c_int(demb.shape[1]),
                                          c_int(demb.shape[0]), _p(demb), c_int(L), c_int(seq_stride), c_int(seq_off),
                                          _stream()), "cclip_embed_scatter_add")
        return
    V, D = demb.shape
    order, st, cend, cidx, rlen = tables if tables is not None else embed_scatter_tables(text_i32, V, rows=rows, keep=keep)
    n = rows
    # one slot per CHUNK (a run of <= 64 equal ids), touched by multi-chunk runs only; slot = id + (chunk start >> 6)
    # (cclip_embed_tables).  `scratch(n_floats)` (the stack's grow-only scratch) keeps it out of the allocator: round 2 drew a
    # fresh [rows, D] fp32 tensor - 161 MB at bs 1024 - per backward pass.
    slots = V + n // _SEG_CHUNK + 1
    partial = scratch(slots * D) if scratch is not None else torch.empty(slots * D, device=text_i32.device, dtype=torch.float32)
    check(lib.cclip_embed_segsum(_p(order), _p(st), _p(cend), _p(cidx), _p(rlen), c_int(n), _p(dx), c_long(dx.stride(-2)), c_int(D),
                                 _p(demb), c_int(L), c_int(seq_stride), c_int(seq_off), _p(partial), _stream()), "cclip_embed_segsum")


def caption_embed(prefix_proj, ids_i32, wte, wpe, x, *, B: int, P: int, Lt: int) -> None:
    _req(prefix_proj, torch.float32, "prefix_proj")
    assert prefix_proj.is_contiguous() and prefix_proj.numel() == B * P * wte.shape[1], "prefix_proj must be dense [B, P*D]"
    check(lib.cclip_caption_embed(_p(prefix_proj), _p(ids_i32), _p(wte), _p(wpe), c_int(B), c_int(P), c_int(Lt),
                                  c_int(wte.shape[1]), c_int(wte.shape[0]), _p(x), _stream()), "cclip_caption_embed")


def add_positional(emb, wpe, x, *, rows: int, S: int) -> None:
    check(lib.cclip_add_positional(_p(emb), _p(wpe), c_int(rows), c_int(S), c_int(wpe.shape[1]), _p(x), _stream()),
          "cclip_add_positional")


def caption_prompt(feat, prompts, head_start, logit_scale, table, probs, index, ids) -> None:
    """The zero-shot heads over N image feature rows and the attribute ids their arg-maxes select, in one launch
    (cclip_caption_prompt): feat fp32 [N, E] (rows may be strided), prompts fp32 [K, E] of len(head_start) - 1 heads laid one
    after another, head_start a host sequence of ints (head g = prompt rows [head_start[g], head_start[g+1])), logit_scale a
    device scalar holding log(scale), table int32 [prod K_g, A].  Fills probs fp32 [N, K] (softmax per head), index int32
    [N, G] (arg-max per head, the lowest index on a tie) and ids int32 [N, A] = table[combination of the arg-maxes]."""
    for t, name in ((feat, "feat"), (prompts, "prompts"), (logit_scale, "logit_scale"), (probs, "probs")):
        _req(t, torch.float32, name)
    for t, name in ((table, "table"), (index, "index"), (ids, "ids")):
        _req(t, torch.int32, name)
    hs = [int(v) for v in head_start]
    G = len(hs) - 1
    N, E = feat.shape
    K = prompts.shape[0]
    A = table.shape[1]
    assert feat.stride(1) == 1 and prompts.is_contiguous() and prompts.shape[1] == E and table.is_contiguous()
    assert logit_scale.numel() == 1
    assert probs.is_contiguous() and probs.shape == (N, K) and index.is_contiguous() and index.shape == (N, max(G, 0))
    assert ids.is_contiguous() and ids.shape == (N, A)
    arr = (c_int * (G + 1))(*hs) if G >= 0 else None
    check(lib.cclip_caption_prompt(_p(feat), c_long(feat.stride(0)), c_int(N), c_int(E), _p(prompts), c_int(K), arr, c_int(G),
                                   _p(logit_scale), _p(table), c_int(table.shape[0]), c_int(A), _p(probs), _p(index), _p(ids),
                                   _stream()), "cclip_caption_prompt")


def colsum_ws_floats(R: int, C: int) -> int:
    return lib.cclip_colsum_ws_floats(c_int(R), c_int(C))


def colsum(inp: torch.Tensor, out: torch.Tensor, ws: torch.Tensor, *, R: int, C: int, ld: int, accumulate: bool = False):
    check(_fn("cclip_colsum", inp)(_p(inp), c_int(_is16(inp)), c_long(ld), c_int(R), c_int(C), _p(out),
                           c_int(int(accumulate)), _p(ws), _stream()), "cclip_colsum")


# --------------------------------------------------------------------------------------------
# loss side
# --------------------------------------------------------------------------------------------
def l2norm_fwd(x, y, inv_norm) -> None:
    check(lib.cclip_l2norm_fwd(_p(x), c_long(x.stride(0)), c_int(x.shape[0]), c_int(x.shape[1]), _p(y), c_long(y.stride(0)),
                               _p(inv_norm), _stream()), "cclip_l2norm_fwd")


def l2norm_bwd(dy, y, inv_norm, dx, mul_dev=None) -> None:
    check(lib.cclip_l2norm_bwd(_p(dy), c_long(dy.stride(0)), _p(y), c_long(y.stride(0)), _p(inv_norm), c_int(y.shape[0]),
                               c_int(y.shape[1]), _p(dx), c_long(dx.stride(0)), _p(mul_dev), _stream()), "cclip_l2norm_bwd")


def xent_rows(logits, labels_i32, *, loss_row=None, pred=None, dlogits=None, grad_scale: float = 1.0,
              ignore_index: int = -100, rowdot=None) -> None:
    _req(logits, torch.float32, "logits"); _req(labels_i32, torch.int32, "labels")
    R, C = logits.shape
    check(_fn("cclip_xent_rows", dlogits)(_p(logits), c_long(logits.stride(0)), c_int(R), c_int(C), _p(labels_i32), c_int(ignore_index),
                              c_float(grad_scale), _p(loss_row), _p(pred), _p(dlogits),
                              c_int(_is16(dlogits)),
                              c_long(0 if dlogits is None else dlogits.stride(0)), _p(rowdot), _stream()), "cclip_xent_rows")


_PER_ROW = dict(loss_row=torch.float32, pred=torch.int32, hit=torch.float32, agree=torch.float32, rowdot=torch.float32,
                rowsum=torch.float32)


def _loss_rows(logits, dlogits, *, classes=None, teacher=None, **per_row):
    """The arguments the fp32 row losses share (xent_rows_classes, sigmoid_rows, kl_rows): fp32 logits [R, C] with unit column
    stride; `classes`, the int32 class vectors ([R], [C]) of the class-vector losses; `teacher`, the second fp32 [R, C]
    operand of kl_rows on the same device (unit column stride, a row stride of its own); the optional per-row outputs [R] by
    their names in _PER_ROW; and the optional fp32 gradient, which may be `logits` itself.  Returns (R, C)."""
    _req(logits, torch.float32, "logits")
    for t, name in zip(classes or (), ("row_class", "col_class")):
        _req(t, torch.int32, name)
    if teacher is not None:
        _req(teacher, torch.float32, "teacher")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError(f"logits: expected [R, C] with unit column stride, got {tuple(logits.shape)} strides {logits.stride()}")
    R, C = logits.shape
    for t, n, name in zip(classes or (), (R, C), ("row_class", "col_class")):
        if t.shape != (n,) or not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous [{n}], got {tuple(t.shape)}")
    if teacher is not None and (teacher.shape != (R, C) or teacher.stride(1) != 1 or teacher.device != logits.device):
        raise ValueError(f"teacher: expected [{R}, {C}] with unit column stride on {logits.device}, got {tuple(teacher.shape)} "
                         f"strides {teacher.stride()} on {teacher.device}")
    for name, t in per_row.items():
        if t is not None:
            _req(t, _PER_ROW[name], name)
            if t.shape != (R,) or not t.is_contiguous():
                raise ValueError(f"{name}: expected contiguous [{R}], got {tuple(t.shape)}")
    if dlogits is not None:
        _req(dlogits, torch.float32, "dlogits")
        if dlogits.shape != (R, C) or dlogits.stride(1) != 1:
            raise ValueError(f"dlogits: expected [{R}, {C}] with unit column stride, got {tuple(dlogits.shape)}")
    return R, C


def xent_rows_classes(logits, row_class_i32, col_class_i32, *, loss_row=None, pred=None, hit=None, dlogits=None,
                      grad_scale: float = 1.0, rowdot=None) -> None:
    """Class-aware row cross-entropy (include/cclip_hip.h, cclip_xent_rows_classes): the positives of row r are the columns
    whose class equals row_class[r]; a negative class id is 'unlabelled'.  fp32 only; dlogits may be `logits` itself."""
    R, C = _loss_rows(logits, dlogits, classes=(row_class_i32, col_class_i32), loss_row=loss_row, pred=pred, hit=hit, rowdot=rowdot)
    check(lib.cclip_xent_rows_classes(_p(logits), c_long(logits.stride(0)), c_int(R), c_int(C), _p(row_class_i32),
                                      _p(col_class_i32), c_float(grad_scale), _p(loss_row), _p(pred), _p(hit), _p(dlogits),
                                      c_long(0 if dlogits is None else dlogits.stride(0)), _p(rowdot), _stream()),
          "cclip_xent_rows_classes")


def sigmoid_rows(logits, row_class_i32, col_class_i32, bias, *, loss_row=None, pred=None, hit=None, dlogits=None,
                 grad_scale: float = 1.0, rowdot=None, rowsum=None) -> None:
    """Pairwise sigmoid (SigLIP) row loss (include/cclip_hip.h, cclip_sigmoid_rows): cell (r, c) is a positive when column c
    carries row r's class, a negative otherwise; a negative class id is 'unlabelled'.  `bias` is a one-element fp32 device
    tensor (never read on the host).  fp32 only; dlogits may be `logits` itself; rowdot / rowsum come only with dlogits."""
    _req(bias, torch.float32, "bias")
    if bias.numel() != 1:
        raise ValueError(f"bias: expected one element, got {tuple(bias.shape)}")
    R, C = _loss_rows(logits, dlogits, classes=(row_class_i32, col_class_i32), loss_row=loss_row, pred=pred, hit=hit, rowdot=rowdot,
                      rowsum=rowsum)
    if dlogits is None and (rowdot is not None or rowsum is not None):
        raise ValueError("rowdot / rowsum are written only together with dlogits")
    check(lib.cclip_sigmoid_rows(_p(logits), c_long(logits.stride(0)), c_int(R), c_int(C), _p(row_class_i32), _p(col_class_i32),
                                 _p(bias), c_float(grad_scale), _p(loss_row), _p(pred), _p(hit), _p(dlogits),
                                 c_long(0 if dlogits is None else dlogits.stride(0)), _p(rowdot), _p(rowsum), _stream()),
          "cclip_sigmoid_rows")


def kl_rows(logits, teacher, *, loss_row=None, pred=None, agree=None, dlogits=None, grad_scale: float = 1.0,
            rowdot=None) -> None:
    """Distillation row loss (include/cclip_hip.h, cclip_kl_rows): KL(softmax(teacher row) || softmax(logits row)) per row, its
    gradient w.r.t. `logits`, and whether the two rows' arg-maxes agree.  `teacher` is fp32 [R, C] on the device of `logits`
    with a row stride of its own, and is only read.  fp32 only; dlogits may be `logits` itself; rowdot comes only with
    dlogits."""
    R, C = _loss_rows(logits, dlogits, teacher=teacher, loss_row=loss_row, pred=pred, agree=agree, rowdot=rowdot)
    if dlogits is None and rowdot is not None:
        raise ValueError("rowdot is written only together with dlogits")
    check(lib.cclip_kl_rows(_p(logits), c_long(logits.stride(0)), _p(teacher), c_long(teacher.stride(0)), c_int(R), c_int(C),
                            c_float(grad_scale), _p(loss_row), _p(pred), _p(agree), _p(dlogits),
                            c_long(0 if dlogits is None else dlogits.stride(0)), _p(rowdot), _stream()), "cclip_kl_rows")


def reduce_dot(a, b, out, *, alpha: float = 1.0, mul_dev=None, accumulate: bool = False) -> None:
    check(lib.cclip_reduce_dot(_p(a), _p(b), c_long(a.numel()), c_float(alpha), _p(mul_dev), _p(out),
                               c_int(int(accumulate)), _stream()), "cclip_reduce_dot")


# --------------------------------------------------------------------------------------------
# optimiser / casts over flat buffers
# --------------------------------------------------------------------------------------------
def adamw_step(param, grad, exp_avg, exp_avg_sq, *, lr: float, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0,
               step: int = 1, correct_bias: bool = True, grad_scale: float = 1.0, mode: int = 0, bf16_shadow=None):
    n = param.numel()
    check(_fn("cclip_adamw_step", bf16_shadow)(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), c_long(n), c_float(lr), c_float(beta1),
                               c_float(beta2), c_float(eps), c_float(weight_decay), c_int(step), c_int(int(correct_bias)),
                               c_float(grad_scale), c_int(mode), _p(bf16_shadow), _stream()), "cclip_adamw_step")


def adamw_grid(n: int) -> int:
    """blocks of the adamw_step / adamw_step_groups launch over n elements (0 for an n they refuse)"""
    return _query("cclip_adamw_grid", c_int, c_long(n))


def sumsq_workspace(n: int) -> int:
    """bytes of scratch `sumsq` needs for n elements: 4 per first-stage block (0 for an n it refuses)"""
    return _query("cclip_sumsq_workspace", c_long, c_long(n))


def sumsq(x, *, out=None, accumulate: bool = False, nonfinite_count=None, workspace=None):
    """out (+)= sum of x[i]^2 over a flat fp32 device range (include/cclip_hip.h, cclip_sumsq_f32): two launches, no atomics,
    equal bits from equal data.  out: fp32 [1] on x's device (allocated when None; read first when `accumulate`);
    nonfinite_count: int32 [1], raised by one when out ends up inf or NaN; workspace: fp32, at least sumsq_workspace(n) bytes.
    Returns out.  Nothing is read on the host."""
    f = "sumsq"
    _dev_tensor(f, x, "x", torch.float32, 1, None)
    dev, n = x.device, x.numel()
    if accumulate and out is None:
        raise ValueError(f"{f}: accumulate needs the `out` to add to")
    out = _out(f, out, "out", torch.float32, (1,), dev)
    _dev_tensor(f, nonfinite_count, "nonfinite_count", torch.int32, (1,), dev, optional=True)
    if n <= 0 or n % 4:
        raise ValueError(f"{f}: x must hold a positive multiple of 4 elements, got {n}")
    if x.data_ptr() % 16:
        raise ValueError(f"{f}: x must be 16-byte aligned (address % 16 = {x.data_ptr() % 16})")
    ws = _workspace(f, workspace, sumsq_workspace(n), torch.float32, dev, flat=True)
    check(lib.cclip_sumsq_f32(_p(x), c_long(n), _p(ws), _p(out), c_int(int(accumulate)), _p(nonfinite_count), _stream()),
          "cclip_sumsq_f32")
    return out


def adamw_step_groups(param, grad, exp_avg, exp_avg_sq, chunk_group, *, lrs, weight_decays, beta1=0.9, beta2=0.999, eps=1e-6,
                      step: int = 1, correct_bias: bool = True, grad_scale: float = 1.0, mode: int = 0, bf16_shadow=None,
                      sumsq_dev=None, max_norm=None, skip_nonfinite: bool = False, ema=None, ema_decay: float = 0.0) -> None:
    """adamw_step with parameter groups, norm clipping from a device scalar and EMA weights, in one launch
    (include/cclip_hip.h, cclip_adamw_step_groups).  param / grad / exp_avg / exp_avg_sq (/ ema): flat fp32 of n elements,
    n % 4 == 0, 16-byte aligned; chunk_group: uint8 [ceil(n / 64)] on the same device, the group of every 64-element chunk of
    THIS range (a slice of the arena's table); lrs / weight_decays: host sequences, one entry per group (at most 256) - a table
    entry beyond them is the caller's to avoid and is not checked here (it would need a read-back).  sumsq_dev: fp32 [1], the sum
    of squares of the unscaled gradients (`sumsq`), with max_norm finite and > 0; skip_nonfinite: a non-finite scalar makes the
    launch write nothing.  bf16_shadow: the 16-bit copy of param (either operand dtype), rewritten in the same pass."""
    f = "adamw_step_groups"
    _dev_tensor(f, param, "param", torch.float32, 1, None)
    dev, n = param.device, param.numel()
    _dev_tensors(f, dev, ((grad, "grad", torch.float32, (n,), False), (exp_avg, "exp_avg", torch.float32, (n,), False),
                          (exp_avg_sq, "exp_avg_sq", torch.float32, (n,), False),
                          (chunk_group, "chunk_group", torch.uint8, ((n + 63) // 64,), False),
                          (bf16_shadow, "bf16_shadow", HALF_TYPES, (n,), True), (sumsq_dev, "sumsq_dev", torch.float32, (1,), True),
                          (ema, "ema", torch.float32, (n,), True)))
    lrs, wds = [float(x) for x in lrs], [float(x) for x in weight_decays]
    if not 1 <= len(lrs) <= 256 or len(wds) != len(lrs):
        raise ValueError(f"{f}: lrs and weight_decays must have one entry per group, 1 to 256 groups, got {len(lrs)} and {len(wds)}")
    if n <= 0 or n % 4:
        raise ValueError(f"{f}: param must hold a positive multiple of 4 elements, got {n}")
    if step < 1:
        raise ValueError(f"{f}: step must be >= 1, got {step}")
    if sumsq_dev is not None:
        if max_norm is None or not 0.0 < _finite(f, "max_norm", max_norm) <= 3.4028234e38:
            raise ValueError(f"{f}: max_norm must be finite and > 0 when sumsq_dev is given, got {max_norm}")
    elif max_norm is not None or skip_nonfinite:
        raise ValueError(f"{f}: max_norm and skip_nonfinite need the device scalar `sumsq_dev`")
    if ema is not None and not 0.0 <= float(ema_decay) <= 1.0:
        raise ValueError(f"{f}: ema_decay must lie in [0, 1], got {ema_decay}")
    for t, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (ema, "ema")):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"{f}: {nm} must be 16-byte aligned (address % 16 = {t.data_ptr() % 16})")
    if bf16_shadow is not None and bf16_shadow.data_ptr() % 8:
        raise ValueError(f"{f}: bf16_shadow must be 8-byte aligned (address % 8 = {bf16_shadow.data_ptr() % 8})")
    G = len(lrs)
    check(_fn("cclip_adamw_step_groups", bf16_shadow)(
        _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), c_long(n), _p(chunk_group), (c_float * G)(*lrs), (c_float * G)(*wds),
        c_int(G), c_float(beta1), c_float(beta2), c_float(eps), c_int(step), c_int(int(correct_bias)), c_float(grad_scale),
        c_int(mode), _p(bf16_shadow), _p(sumsq_dev), c_float(0.0 if max_norm is None else max_norm), c_int(int(skip_nonfinite)),
        _p(ema), c_float(ema_decay), _stream()), "cclip_adamw_step_groups")


def transpose16_batched(src_base: torch.Tensor, dst_base: torch.Tensor, table_dev: torch.Tensor, max_tiles: int) -> None:
    """table_dev: int64 [n, 4] on the device = (src element offset, dst element offset, rows, cols) per matrix"""
    assert src_base.dtype in HALF_TYPES and dst_base.dtype == src_base.dtype and table_dev.dtype == torch.int64 and table_dev.is_cuda
    check(lib.cclip_transpose16_batched(_p(src_base), _p(dst_base), _p(table_dev), c_int(table_dev.shape[0]), c_int(max_tiles),
                                        _stream()), "cclip_transpose16_batched")


def scale_f32(x: torch.Tensor, alpha: float) -> None:
    """x *= alpha in place (flat fp32, numel % 4 == 0, 16-byte aligned)"""
    _req(x, torch.float32, "x")
    assert x.is_contiguous()
    check(lib.cclip_scale_f32(_p(x), c_long(x.numel()), c_float(alpha), _stream()), "cclip_scale_f32")


def cast_f32_to_bf16(src, dst) -> None:
    check(_fn("cclip_cast_f32_to_bf16", dst)(_p(src), _p(dst), c_long(src.numel()), _stream()), "cclip_cast_f32_to_bf16")


CONCEPT_MAX_V = 1 << 24


def concept_codes_workspace(N: int, V: int, D: int) -> int:
    """bytes of workspace cclip_concept_codes needs (the fp32 w_{k-1} of every row: 4 N * 4 ceil(V / 4); 0 for a problem it
    would refuse)"""
    return _query("cclip_concept_codes_workspace", c_long, c_long(N), c_long(V), c_int(D))


def concept_codes(x, c, l1: float, eta: float, iters: int, *, out_w=None, workspace=None):
    """Sparse non-negative codes of the rows of x [N, D] over the dictionary c [V, D] (both 16-bit unit rows of one dtype under
    the contract of kmeans_assign): `iters` FISTA iterations of  min_{w >= 0} 1/2 |x - w c|^2 + l1 sum w  with step eta (1 / the
    largest eigenvalue of c^T c) and beta_k = k / (k + 3), all inside one launch (include/cclip_hip.h, cclip_concept_codes).
    Returns (w fp32 [N, V], resid2 fp32 [N], l1norm fp32 [N], nnz int32 [N], delta fp32 [N], kkt fp32 [N]): the read-outs are
    taken at w itself; kkt is the row's distance from optimality.  out_w: an fp32 [N, V] device view with inner stride 1, a row
    stride that is a multiple of 4 and 16-byte alignment (nothing is written between its rows); workspace: a contiguous fp32
    device tensor of at least concept_codes_workspace(N, V, D) bytes.  1 <= V <= 2^24, D % 32 == 0, 32 <= D <= 1024, N < 2^31.
    A row's outputs depend on neither N nor its position; two calls are bitwise equal.  No host read."""
    fname = "concept_codes"
    N, V, D, ldx, ldc = _kmeans_operands(fname, x, c, "c")
    if V > CONCEPT_MAX_V:
        raise NotImplementedError(f"{fname}: V = {V}; the kernel takes up to {CONCEPT_MAX_V} concepts")
    l1, eta = _finite(fname, "l1", l1, nonneg=True), _finite(fname, "eta", eta, nonneg=True)
    if isinstance(iters, bool) or int(iters) != iters or iters < 0:
        raise ValueError(f"{fname}: iters = {iters!r} must be an integer >= 0")
    dev = x.device
    if out_w is None:
        out_w = torch.empty(N, (V + 3) // 4 * 4, device=dev, dtype=torch.float32)[:, :V]
    else:
        _dev_tensor(fname, out_w, "out_w", torch.float32, (N, V), dev, contiguous=False, host_error=ValueError, dtype_error=ValueError)
        if out_w.stride(1) != 1:
            raise ValueError(f"{fname}: out_w must have inner stride 1, got strides {out_w.stride()}")
    # a one-row out_w: its stride is raised to the 4 ceil(V / 4) the kernel needs but, unlike _ld16's, not rounded down to a multiple
    ldw = _ld(out_w, multiple=1, at_least=(V + 3) // 4 * 4)
    if ldw % 4 or ldw < V or out_w.data_ptr() % 16:
        raise ValueError(f"{fname}: out_w must be 16-byte aligned with a row stride >= V that is a multiple of 4 elements "
                         f"(stride {out_w.stride(0)}, address % 16 = {out_w.data_ptr() % 16})")
    workspace = _workspace(fname, workspace, concept_codes_workspace(N, V, D), torch.float32, dev, align16=True)
    resid2, l1norm, delta, kkt = (torch.empty(N, device=dev, dtype=torch.float32) for _ in range(4))
    nnz = torch.empty(N, device=dev, dtype=torch.int32)
    fn = _fn("cclip_concept_codes", x, c)
    check(fn(_p(x), c_long(ldx), c_long(N), _p(c), c_long(ldc), c_long(V), c_int(D), c_float(l1), c_float(eta), c_int(int(iters)),
             _p(out_w), c_long(ldw), _p(resid2), _p(l1norm), _p(nnz), _p(delta), _p(kkt), _p(workspace),
             c_long(workspace.numel() * 4), _stream()), "cclip_concept_codes")
    return out_w, resid2, l1norm, nnz, delta, kkt


MOMENTS_MAX_C = 256
GAUSS_MAX_R = 1024
GAUSS_MAX_C = 256


def moments_parts(N: int, C: int, D: int) -> int:
    """the number of parts cclip_class_moments splits the rows into: a function of (N, C, D) alone (0 for a refused problem)"""
    return _query("cclip_moments_parts", c_int, c_long(N), c_int(C), c_int(D))


def moments_workspace(N: int, C: int, D: int) -> int:
    """bytes of workspace cclip_class_moments needs (the partial 128 x 128 blocks of every part and the non-finite flags:
    include/cclip_hip.h states the closed form; 0 for a problem it would refuse)"""
    return _query("cclip_moments_workspace", c_long, c_long(N), c_int(C), c_int(D))


def class_moments(x, labels, C: int, *, out=None, workspace=None):
    """Second moments of the rows of x [N, D] (16-bit, under the contract of kmeans_assign) by class: labels int32 [N] or None
    (every row is class 0; C must be 1).  Returns (count int32 [C], sum fp32 [C, D], gram fp32 [D, D]): rows per class, the sum of
    each class's rows, and the sum of x^T x over the live rows; a row whose label lies outside [0, C) is dropped from all three.
    Products are exact, every entry is an fp32 sum over moments_parts(N, C, D) chains merged in a fixed tree; gram is bitwise
    symmetric; two calls are bitwise equal.  `out`: (count, sum, gram) to write into; workspace: a contiguous fp32 device tensor
    of at least moments_workspace(N, C, D) bytes, 16-byte aligned.  1 <= C <= 256, D % 32 == 0, 32 <= D <= 1024, N < 2^31.
    Enqueues three launches; no host read."""
    fname = "class_moments"
    _view16(fname, ((x, "x", HALF_TYPES, None, False),))
    (N, D), dev = x.shape, x.device
    _dev_tensors(fname, dev, ((labels, "labels", torch.int32, (N,), True),), host_error=ValueError, dtype_error=ValueError)
    if isinstance(C, bool) or int(C) != C:
        raise ValueError(f"{fname}: C = {C!r} must be an integer")
    C = int(C)
    _limits16(fname, D, "N", (N,))
    if not 1 <= C <= MOMENTS_MAX_C:
        raise NotImplementedError(f"{fname}: C = {C}; the kernel takes 1 .. {MOMENTS_MAX_C} classes")
    if labels is None and C != 1:
        raise ValueError(f"{fname}: without labels every row is class 0: C must be 1, got {C}")
    ldx = _ld16(fname, x, "x")
    o = tuple(out) if out is not None else (None, None, None)
    if len(o) != 3:
        raise ValueError(f"{fname}: out must be (count, sum, gram)")
    count = _out(fname, o[0], "count", torch.int32, (C,), dev)
    csum = _out(fname, o[1], "sum", torch.float32, (C, D), dev)
    gram = _out(fname, o[2], "gram", torch.float32, (D, D), dev)
    nbytes = moments_workspace(N, C, D)
    workspace = _workspace(fname, workspace, nbytes, torch.float32, dev, align16=True)
    fn = _fn("cclip_class_moments", x)
    check(fn(_p(x), c_long(ldx), c_long(N), c_int(D), _p(labels), c_int(C), _p(count), _p(csum), _p(gram), _p(workspace),
             c_long(workspace.numel() * 4), _stream()), "cclip_class_moments")
    return count, csum, gram


def gauss_scores_workspace(R: int, D: int) -> int:
    """bytes of workspace cclip_gauss_scores needs (the hi + lo image of T: 4 * 16 ceil(R / 16) * D; 0 for refused sizes)"""
    return _query("cclip_gauss_scores_workspace", c_long, c_long(R), c_int(D))


def gauss_scores(x, T, *, t0=None, centres=None, offset=None, want_d2: bool = False, want_z: bool = False, out=None):
    """z = (T_hi + T_lo) x - t0 for every row of x [Q, D] (16-bit, under the contract of kmeans_assign) with T fp32 [R, D] and
    t0 fp32 [R] or None, then with centres fp32 [C, R] and offset fp32 [C] or None:
        d2[q, c] = sum_r (z[q, r] - centres[c, r])^2     score[q, c] = -0.5 d2[q, c] + offset[c]
    in fp32 as include/cclip_hip.h states (cclip_gauss_scores; never the expanded form).  Returns (pred int32 [Q], lse fp32 [Q],
    nearest int32 [Q], dmin fp32 [Q], d2 fp32 [Q, C] or None, z fp32 [Q, R] or None): argmax and logsumexp of the scores (ties to
    the lower class, NaN lowest), argmin and min of d2; d2 and z only when asked for.  With centres=None only z is computed (the
    PCA transform) and the first five are None.  `out`: a tuple of six tensors (or None) to write those into.  A row's outputs
    depend on neither Q nor its position; two calls are bitwise equal.  1 <= R <= 1024, 1 <= C <= 256, D % 32 == 0,
    32 <= D <= 1024.  Enqueues two launches; no host read."""
    fname = "gauss_scores"
    _dev_tensors(fname, None, ((x, "x", None, None, False), (T, "T", None, None, False)), contiguous=False)   # cuda, both operands, first
    _view16(fname, ((x, "x", HALF_TYPES, None, False),))
    (Q, D), dev = x.shape, x.device
    R = _dev_tensor(fname, T, "T", torch.float32, (None, D), dev, device_error=TypeError).shape[0]
    _dev_tensors(fname, dev, ((t0, "t0", torch.float32, (R,), True), (centres, "centres", torch.float32, (None, R), True)),
                 host_error=ValueError, dtype_error=ValueError)
    C = 0 if centres is None else centres.shape[0]
    _dev_tensors(fname, dev, ((offset, "offset", torch.float32, (C,), True),), host_error=ValueError, dtype_error=ValueError)
    if centres is None and (offset is not None or want_d2):
        raise ValueError(f"{fname}: offset and want_d2 need centres")
    _limits16(fname, D, "Q", (Q,))
    if not 1 <= R <= GAUSS_MAX_R:
        raise NotImplementedError(f"{fname}: R = {R}; the kernel takes 1 .. {GAUSS_MAX_R} transform rows")
    if centres is not None and not 1 <= C <= GAUSS_MAX_C:
        raise NotImplementedError(f"{fname}: C = {C}; the kernel takes 1 .. {GAUSS_MAX_C} centres")
    ldx = _ld16(fname, x, "x")
    o = tuple(out) if out is not None else (None,) * 6
    if len(o) != 6:
        raise ValueError(f"{fname}: out must be (pred, lse, nearest, dmin, d2, z), None where nothing is provided")
    pred = lse = nearest = dmin = d2 = z = None
    if centres is not None:
        pred = _out(fname, o[0], "pred", torch.int32, (Q,), dev)
        lse = _out(fname, o[1], "lse", torch.float32, (Q,), dev)
        nearest = _out(fname, o[2], "nearest", torch.int32, (Q,), dev)
        dmin = _out(fname, o[3], "dmin", torch.float32, (Q,), dev)
        if want_d2 or o[4] is not None:
            d2 = _out(fname, o[4], "d2", torch.float32, (Q, C), dev)
    if centres is None or want_z or o[5] is not None:
        z = _out(fname, o[5], "z", torch.float32, (Q, R), dev)
    nbytes = gauss_scores_workspace(R, D)
    ws = _workspace(fname, None, nbytes, torch.float32, dev)
    fn = _fn("cclip_gauss_scores", x)
    check(fn(_p(x), c_long(ldx), c_long(Q), c_int(D), _p(T), _p(t0), c_int(R), _p(centres), _p(offset), c_int(C), _p(pred), _p(lse),
             _p(nearest), _p(dmin), _p(d2), _p(z), _p(ws), c_long(nbytes), _stream()), "cclip_gauss_scores")
    return pred, lse, nearest, dmin, d2, z
