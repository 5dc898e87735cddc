"""Equivalence record of clip/loss.py across a change that must alter neither what it launches nor what it returns (a refactor
of the loss Functions): for seeded inputs, the ordered launcher calls and collectives of every case, and every result.

    python tools/loss_dump.py [--cpu] --out before.pt        # on the tree to compare against
    python tools/loss_dump.py [--cpu] --compare before.pt    # on the new tree: exit status 1 at the first difference

The `ops` and `dist` names that clip.loss sees are wrapped by a recorder.  A trace entry is the call's name and its arguments
by parameter name (defaults filled in): scalars as they are, every tensor as shape, stride, dtype, storage offset and a storage
number given by first appearance within the case - so packing (column halves of one buffer) and aliasing (the gradient written
over the logits) show.  Results: loss, stats and the gradients of image features, text features, logit_scale and logit_bias.

Cases (E = 16): contrastive_loss and sigmoid_loss, each pairwise (N = 8), class-aware square (N = 8, repeated classes, one -1)
and class-aware rectangular (N = 8, M = 5, text_labels with a -1); each under no_grad, with everything requiring a gradient
(upstream 2.0) and with only logit_scale / logit_bias requiring one; labels as int64 and as int32; and the refused calls with
their exception type and message.  Without --cpu all of this runs on the built library on cuda:0.  With --cpu it runs on
tests/cpu_ops_shim.py, and the four square forms also at N_loc = 4 in two gloo processes (rank 0's record is kept), with the
rectangular call that a live group refuses.  Traces must be equal and results torch.equal: the arithmetic is the same calls in
the same order, on the shim and on the device alike."""
import argparse
import contextlib
import inspect
import os
import sys
import tempfile
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.join(ROOT, "tests")]

E, N, M = 16, 8, 5
SQUARE = [0, 1, 2, 0, -1, 2, 2, 1]
RECT = ([0, 3, 2, 0, 1, 2, 2, 4], [2, 0, -1, 1, 0])                 # classes 3 and 4 have no text; one unlabelled column
FORMS = (("pairwise", N, None, None), ("square", N, SQUARE, None), ("rect", M, RECT[0], RECT[1]))
MODES = ("no_grad", "all", "scalars")
COLLECTIVES = ("all_gather_into_tensor", "all_gather", "all_reduce", "reduce_scatter_tensor", "reduce_scatter", "broadcast",
               "all_to_all_single")


class Recorder:
    """the ordered calls of one case through the namespaces it wraps"""

    def __init__(self):
        self.begin()

    def begin(self):
        self.trace, self._number, self._alive = [], {}, []

    def wrap(self, target, names=None):
        rec = self

        class Proxy:
            def __getattr__(self, name):                            # looked up at call time, as clip.loss must
                f = getattr(target, name)
                if not callable(f) or isinstance(f, type) or (names is not None and name not in names):
                    return f
                return lambda *a, **kw: rec.call(name, f, a, kw)
        return Proxy()

    def call(self, name, f, args, kw):
        bound = inspect.signature(f).bind(*args, **kw)
        bound.apply_defaults()
        self.trace.append((name, {k: self.describe(v) for k, v in bound.arguments.items()}))
        return f(*args, **kw)

    def describe(self, v):
        if isinstance(v, torch.Tensor):
            storage = v.untyped_storage()
            if storage.data_ptr() not in self._number:
                self._number[storage.data_ptr()] = len(self._number)
                self._alive.append(storage)                         # held to the end of the case: no address comes twice
            return dict(shape=tuple(v.shape), stride=tuple(v.stride()), dtype=str(v.dtype), offset=v.storage_offset(),
                        storage=self._number[storage.data_ptr()])
        return v if v is None or isinstance(v, (bool, int, float, str)) else type(v).__name__


def cpu_shim():
    """tests/cpu_ops_shim.py - on a tree from before it was the one shim, with the two row losses the helper files then held"""
    import cpu_ops_shim
    if hasattr(cpu_ops_shim, "sigmoid_rows"):
        return cpu_ops_shim
    import class_loss_helpers
    import sigmoid_loss_helpers
    return types.SimpleNamespace(**vars(cpu_ops_shim), xent_rows_classes=class_loss_helpers.xent_rows_classes,
                                 sigmoid_rows=sigmoid_loss_helpers.sigmoid_rows)


def instrument(cpu):
    import clip.loss as closs
    rec = Recorder()
    closs.ops = rec.wrap(cpu_shim() if cpu else closs.ops)
    closs.dist = rec.wrap(closs.dist, COLLECTIVES)
    return closs, rec


def inputs(seed, rows):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, E, generator=g), torch.randn(rows, E, generator=g)


def as_labels(ids, dtype, sl=slice(None)):
    return None if ids is None else torch.tensor(ids, dtype=dtype)[sl]


def run(closs, rec, dev, entry, fi, ft, mode, **kw):
    """one call (and its backward): {trace, loss, stats, dfi, dft, dls, dlb}, or {trace, error} where it is refused"""
    fi, ft = (x.clone().to(dev).requires_grad_(mode == "all") for x in (fi, ft))
    ls, lb = (torch.tensor(v, device=dev).requires_grad_(mode != "no_grad") for v in (1.3, -1.5))
    scalars = (ls,) if entry == "contrastive" else (ls, lb)
    rec.begin()
    try:
        with torch.no_grad() if mode == "no_grad" else contextlib.nullcontext():
            loss, stats = getattr(closs, entry + "_loss")(fi, ft, *scalars, **kw)
        if mode != "no_grad":
            (loss * 2.0).backward()
    except Exception as e:  # noqa: BLE001 - the refusal is the record
        return dict(trace=rec.trace, error=(type(e).__name__, str(e)))
    res = dict(loss=loss, stats=stats, dfi=fi.grad, dft=ft.grad, dls=ls.grad, dlb=lb.grad)
    return dict(trace=rec.trace, **{k: None if v is None else v.detach().cpu() for k, v in res.items()})


def refused(cpu):
    """(name, entry, rows of the text side, keyword arguments) of the calls that must raise"""
    i64, f32 = torch.int64, torch.float32
    for entry in ("contrastive", "sigmoid"):
        yield "text_labels_without_labels", entry, N, dict(text_labels=torch.zeros(N, dtype=i64))
        yield "text_labels_without_labels_and_unequal_rows", entry, M, dict(text_labels=torch.zeros(M, dtype=i64))
        yield "square_unequal_rows", entry, M, dict(labels=as_labels(SQUARE, i64))
        if entry == "sigmoid" or cpu:       # contrastive_loss leaves this one to the launchers: the shim raises, the device must not see it
            yield "pairwise_unequal_rows", entry, M, {}
        yield "labels_dtype", entry, N, dict(labels=torch.zeros(N, dtype=f32))
        yield "labels_dtype_and_unequal_rows", entry, M, dict(labels=torch.zeros(N, dtype=f32))
        yield "text_labels_dtype", entry, M, dict(labels=as_labels(RECT[0], i64), text_labels=torch.zeros(M, dtype=f32))
        yield "labels_shape", entry, N, dict(labels=torch.zeros(N - 1, dtype=i64))
        yield "labels_shape_2d", entry, N, dict(labels=torch.zeros(N, 1, dtype=i64))
        yield "labels_shape_and_text_labels_dtype", entry, M, dict(labels=torch.zeros(N + 1, dtype=i64), text_labels=torch.zeros(M, dtype=f32))
        yield "text_labels_shape", entry, M, dict(labels=as_labels(RECT[0], i64), text_labels=torch.zeros(M - 1, dtype=i64))


def single_cases(cpu):
    closs, rec = instrument(cpu)
    dev = torch.device("cpu" if cpu else "cuda:0")
    seed = 0
    for entry in ("contrastive", "sigmoid"):
        for form, rows, a, b in FORMS:
            for dt in (torch.int64, torch.int32) if a is not None else (None,):
                for mode in MODES:
                    seed += 1
                    kw = {} if a is None else dict(labels=as_labels(a, dt), text_labels=as_labels(b, dt))
                    yield f"{entry}/{form}/{str(dt).split('.')[-1]}/{mode}", run(closs, rec, dev, entry, *inputs(seed, rows), mode, **kw)
    for name, entry, rows, kw in refused(cpu):
        yield f"refused/{entry}/{name}", run(closs, rec, dev, entry, *inputs(99, rows), "all", **kw)


def _dp_worker(rank, world, port, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    import clip.parallel as par
    closs, rec = instrument(True)
    par.init_distributed("gloo")
    nloc = N // world
    sl = slice(rank * nloc, (rank + 1) * nloc)
    out, seed = {}, 200
    for entry in ("contrastive", "sigmoid"):
        for form, _, a, _ in FORMS[:2]:
            for mode in MODES:
                seed += 1
                fi, ft = inputs(seed, N)
                kw = {} if a is None else dict(labels=as_labels(a, torch.int64, sl))
                out[f"gloo2/{entry}/{form}/{mode}"] = run(closs, rec, "cpu", entry, fi[sl], ft[sl], mode, **kw)
        fi, ft = inputs(299, N)                                     # refused before any collective, on every rank
        out[f"gloo2/refused/{entry}/text_labels_under_a_group"] = run(
            closs, rec, "cpu", entry, fi[sl], ft[sl], "all", labels=as_labels(SQUARE, torch.int64, sl), text_labels=as_labels(SQUARE, torch.int64, sl))
    if rank == 0:
        torch.save(out, path)
    dist.destroy_process_group()


def dp_cases():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "rank0.pt")
        mp.spawn(_dp_worker, args=(2, 33000 + os.getpid() % 1000, path), nprocs=2, join=True)
        yield from torch.load(path, weights_only=False).items()


def same(old, now):
    if old is None or old.keys() != now.keys():
        return "the record's fields"
    for k, v in now.items():
        o = old[k]
        if isinstance(v, torch.Tensor):
            if not (isinstance(o, torch.Tensor) and o.dtype == v.dtype and o.shape == v.shape and torch.equal(o, v)):
                return k
        elif k == "trace":
            if len(o) != len(v):
                return f"trace: {len(o)} calls saved, {len(v)} made"
            for i, (x, y) in enumerate(zip(o, v)):
                if x != y:
                    return f"trace[{i}]:\n  saved {x}\n  now   {y}"
        elif o != v:
            return f"{k}: saved {o!r}, now {v!r}"
    return None


def main():
    ap = argparse.ArgumentParser()
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--out", help="run the cases and save every trace and result here")
    g.add_argument("--compare", help="run the cases and compare with the record saved here")
    ap.add_argument("--cpu", action="store_true", help="run on tests/cpu_ops_shim.py, the two-process gloo cases included")
    args = ap.parse_args()
    saved = torch.load(args.compare, weights_only=False) if args.compare else {}
    n = calls = 0
    for gen in (single_cases(args.cpu),) + ((dp_cases(),) if args.cpu else ()):
        for name, record in gen:
            if args.compare:
                diff = same(saved.get(name), record)
                if diff:
                    print(f"DIFFERENT  {name}: {diff}", flush=True)
                    sys.exit(1)
            else:
                saved[name] = record
            n += 1
            calls += len(record["trace"])
            tail = f"refused: {record['error'][0]}" if "error" in record else f"{len(record['trace'])} calls"
            print(f"{'same' if args.compare else 'run '}  {name}  ({tail})", flush=True)
    if args.compare:
        if n != len(saved):
            print(f"DIFFERENT  {len(saved)} cases saved, {n} run", flush=True)
            sys.exit(1)
        print(f"{n} cases, {calls} calls: traces equal and results torch.equal to {args.compare}")
    else:
        torch.save(saved, args.out)
        print(f"{n} cases, {calls} calls saved to {args.out}")


if __name__ == "__main__":
    main()
