"""Bit-identity check of the scoring and fp32 row kernels across a change that must not alter their results (a refactor of
csrc/score_tiles.h, score_key.h or row_kernels.h, a compiler update): seeded inputs, every output tensor saved raw.

    python tools/score_dump.py --out before.pt        # on the build to compare against
    python tools/score_dump.py --compare before.pt    # on the new build: exit status 1 at the first tensor that differs

similarity_topk and lm_head_score run in bf16 and fp16 over shapes that reach every kernel variant, both row-tile counts, a
partly empty work-group, row widths that are not a power-of-two number of chunks, padded row strides, a column slice of a
wider buffer, duplicated rows / equal columns, a NaN row, an ignored and an out-of-range label.  xent_rows,
xent_rows_classes, sigmoid_rows and kl_rows: R = 9 over C = 1, 63, 64, 255, 256, 257, 300 (255 .. 257 straddle the four-column
trip of row_kernels.h) without a gradient, with one, and with the gradient written over the logits, every input holding a row of
ties and an all-NaN row; xent_rows also with a 16-bit gradient; kl_rows with a teacher of a row stride of its own that holds
cells at -inf (one of them a lane's first column) and one row equal to the student's.
caption_select: N = 3, K = 1, 5, 64, E = 4, 512, 1024 with references, with and without lm_mean, with a NaN score.
sample_rows: V = 5, 4099, 50257 with top-k, with top-p and with neither, from fixed u.  l2norm_fwd and text_embed: one case.
The other kernels on csrc/score_sweep.h - similarity_range (self-join on and off), kmeans_assign, cache_affinity forward and
backward, probe forward and backward, mreach_nearest and mst_boruvka - run over SWEEP_SHAPES in both dtypes: one D per
dispatch rung and a D that is not a power-of-two number of chunks, 1 / 63 / 65 / 129 operand rows (a partly filled wave, an
idle wave, both row-tile counts), 1 .. 3000 streamed rows (a partial sub-tile, a partial tile, two tiles, several splits), and
one case each with padded row strides.
The kernels on csrc/score_pair.h and the other users of its host contract and of block_sum4 - class_moments, gauss_scores (with
centres and as the PCA transform), concept_codes (0, 1 and 5 iterations over 1, 33 and 75 concepts), kmeans_update, coreset_greedy
(with and without weights), probe forward and backward - run in both dtypes over 1 / 63 / 65 / 257 rows x D = 32, 160, 512, 1024
(every <KSMAX, DS, PRE, MT> variant and a D that is not a power-of-two number of chunks), with 2, 5, 33 and 130 classes dealt so
that every D meets every count (the probe's 1, 2 and 4 class blocks a work-group), one case with padded row strides and one
with a NaN row under an ignored label and an infinity in a live row; tsne_repulsion over 1 .. 3000 points."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "construction-clip_amd")]
from cclip_hip import ops  # noqa: E402

DTYPES = ((torch.bfloat16, "bf16"), (torch.float16, "f16"))
TOPK_SHAPES = [(1, 1, 64, 1), (3, 5, 128, 5), (16, 64, 512, 10), (130, 4097, 128, 10), (100, 1000, 768, 64), (16, 1000, 1024, 10),
               (3, 1000, 32, 5), (100, 1000, 96, 5), (100, 4097, 160, 10)]
LM_SHAPES = [(1, 1, 32), (3, 15, 32), (17, 300, 128), (300, 300, 128), (70, 2050, 512), (65, 4099, 768), (33, 1000, 1024)]
ROW_R, ROW_C = 9, (1, 63, 64, 255, 256, 257, 300)
# (operand rows, streamed rows, D)
SWEEP_SHAPES = [(1, 1, 32), (63, 17, 128), (65, 64, 160), (129, 65, 512), (65, 1025, 768), (129, 3000, 1024), (129, 3000, 128),
                (1, 1025, 512), (63, 3000, 160)]
# rows, D, classes and transform rows of pair_cases
PAIR_ROWS, PAIR_D, PAIR_C, PAIR_T = (1, 63, 65, 257), (32, 160, 512, 1024), (2, 5, 33, 130), (5, 33, 64, 130)


def rnd(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def padded(t, pad):
    """t's values as a view of a buffer whose rows are `pad` elements longer"""
    buf = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def topk_cases():
    for dt, tag in DTYPES:
        for i, (Q, N, D, k) in enumerate(TOPK_SHAPES):
            q, g = rnd(100 + i, Q, D).to(dt).cuda(), rnd(200 + i, N, D).to(dt).cuda()
            yield f"topk/{tag}/{Q}x{N}x{D}k{k}", dict(zip(("scores", "index"), ops.similarity_topk(q, g, k)))
        Q, N, D, k = 130, 4097, 128, 10
        q, g = rnd(150, Q, D).to(dt).cuda(), rnd(250, N, D).to(dt).cuda()
        yield f"topk/{tag}/padded", dict(zip(("scores", "index"), ops.similarity_topk(padded(q, 8), padded(g, 24), k)))
        dup = g.clone()
        dup[1::3] = dup[0:-1:3][:dup[1::3].shape[0]]               # every third row repeats its predecessor: equal scores
        yield f"topk/{tag}/duplicates", dict(zip(("scores", "index"), ops.similarity_topk(q, dup, k)))
        nan = g.clone()
        nan[77] = float("nan")
        yield f"topk/{tag}/nan_row", dict(zip(("scores", "index"), ops.similarity_topk(q, nan, k)))


def lm_cases():
    names = ("logp", "lse", "pred", "pred_logit")
    for dt, tag in DTYPES:
        for i, (R, V, D) in enumerate(LM_SHAPES):
            x, w = rnd(300 + i, R, D).to(dt).cuda(), rnd(400 + i, V, D, scale=0.3).to(dt).cuda()
            labels = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(500 + i)).to(torch.int32).cuda()
            yield f"lm/{tag}/{R}x{V}x{D}", dict(zip(names, ops.lm_head_score(x, w, labels)))
        R, V, D = 70, 2050, 128
        wide = rnd(350, R, D + 64).to(dt).cuda()
        w = rnd(450, V, D, scale=0.3).to(dt).cuda()
        w[1500] = w[20]                                             # two equal columns: the lower one wins a tie
        labels = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(550)).to(torch.int32)
        labels[3], labels[4], labels[5] = -100, V, -1               # ignored; out of range above and below
        yield f"lm/{tag}/slice_labels_equal_columns", dict(zip(names, ops.lm_head_score(wide[:, 32:32 + D], w, labels.cuda())))


def unit(seed, n, D, dt):
    x = rnd(seed, n, D)
    return (x / x.norm(dim=1, keepdim=True)).to(dt).cuda()


def sweep_cases():
    for dt, tag in DTYPES:
        for i, (R, S, D) in enumerate(SWEEP_SHAPES + [SWEEP_SHAPES[3]]):
            pad = i == len(SWEEP_SHAPES)                            # the last case again, with padded row strides
            name = f"{tag}/{R}x{S}x{D}" + ("/padded" if pad else "")
            q, g = unit(1000 + i, R, D, dt), unit(1100 + i, S, D, dt)
            if pad:
                q, g = padded(q, 8), padded(g, 24)
            thr = 1.2 / D ** 0.5                                    # a few percent of the pairs
            yield f"range/{name}", dict(zip(("offsets", "index", "scores"), ops.similarity_range(q, g, thr)))
            yield f"range_self/{name}", dict(zip(("offsets", "index", "scores"), ops.similarity_range(g, g, thr, self_join=True)))
            yield f"kmeans_assign/{name}", dict(zip(("assign", "best", "second"), ops.kmeans_assign(q, g, want_second=True)))
            # few-shot cache over the streamed rows: 5 classes, one of them empty
            gen = torch.Generator().manual_seed(1200 + i)
            labels = torch.randint(0, 4, (S,), generator=gen)
            gather, class_off, class_len = ops.cache_layout(labels, 5)
            keys = torch.zeros(gather.numel(), D, dtype=dt, device="cuda")
            src = g.contiguous()
            keys[(gather >= 0).cuda()] = src[gather[gather >= 0].cuda()]
            keys[(gather < 0).cuda()] = float("nan")                # padding rows are never used
            if pad:
                keys = padded(keys, 16)
            excl = torch.randint(-1, gather.numel(), (R,), generator=gen).to(torch.int32).cuda()
            yield f"cache_affinity/{name}", {"A": ops.cache_affinity(q, keys, class_off, class_len, 5.5, exclude=excl)}
            dA = rnd(1300 + i, R, 5).cuda()
            yield f"cache_affinity_bwd/{name}", {"dG": ops.cache_affinity_backward(q, keys, class_off, class_len, 5.5, dA, exclude=excl)}
            # linear probe: the operand rows against C classes
            C = min(max(2, S // 12), 250)
            W, bias = rnd(1400 + i, C, D, scale=0.5).cuda(), rnd(1500 + i, C).cuda()
            y = torch.randint(-1, C, (R,), generator=gen).to(torch.int32).cuda()
            rw = torch.rand(R, generator=gen).cuda()
            lse, loss, pred, logits = ops.probe_forward(q, W, bias, y, row_weight=rw, logits=True)
            yield f"probe_fwd/{name}", {"lse": lse, "loss": loss, "pred": pred, "logits": logits}
            dW, db, obj = ops.probe_backward(q, W, bias, y, lse, 1.0 / R, 1e-3, row_weight=rw, loss=loss)
            yield f"probe_bwd/{name}", {"dW": dW, "db": db, "objective": obj}
            # mutual reachability over the streamed rows
            core = (torch.rand(S, generator=gen) * 0.5).cuda()
            comp = torch.randint(0, 3, (S,), generator=gen).to(torch.int32).cuda()
            yield f"mreach_nearest/{name}", {"keys": ops.mreach_nearest(g, core, comp)}
            yield f"mst_boruvka/{name}", dict(zip(("u", "v", "m"), ops.mst_boruvka(g, core)))


def pair_cases():
    """the two-product kernels on csrc/score_pair.h and the other users of its host contract and of block_sum4"""
    shapes = [(R, D, PAIR_C[(i + j) % 4], PAIR_T[(i + j) % 4]) for i, R in enumerate(PAIR_ROWS) for j, D in enumerate(PAIR_D)]
    special = (65, 160, 5, 33)
    for dt, tag in DTYPES:
        for i, (R, D, C, Rt) in enumerate(shapes + [special, special]):
            kind = ("", "/padded", "/nan_row")[max(0, i - len(shapes) + 1)]
            name = f"{tag}/{R}x{D}c{C}{kind}"
            gen = torch.Generator().manual_seed(2000 + i)
            x = unit(2100 + i, R, D, dt)
            y = torch.randint(-1, C + 1, (R,), generator=gen).to(torch.int32)       # -1 and C: dropped / ignored rows
            if kind == "/padded":
                x = padded(x, 24)
            if kind == "/nan_row":
                x[7], y[7] = float("nan"), -1                       # ignored by the probe and the moments; gauss, concepts keep it in its row
                x[9, 3] = float("inf")                              # a live row: the moments' flags
                y[9] = 1
            y = y.cuda()
            yield f"class_moments/{name}", dict(zip(("count", "sum", "gram"), ops.class_moments(x, y, C)))
            if i % 4 == 0:
                yield f"class_moments/{name}/no_labels", dict(zip(("count", "sum", "gram"), ops.class_moments(x, None, 1)))
            T, t0 = rnd(2200 + i, Rt, D, scale=0.5).cuda(), rnd(2300 + i, Rt).cuda()
            centres, offset = rnd(2400 + i, C, Rt, scale=0.3).cuda(), rnd(2500 + i, C).cuda()
            names = ("pred", "lse", "nearest", "dmin", "d2", "z")
            yield f"gauss_scores/{name}", dict(zip(names, ops.gauss_scores(x, T, t0=t0, centres=centres, offset=offset, want_d2=True,
                                                                          want_z=True)))
            yield f"gauss_scores/{name}/pca", dict(zip(names, ops.gauss_scores(x, T, want_z=True)))
            for V in (1, 33, 75):
                c = unit(2600 + i + V, V, D, dt)
                for iters in (0, 1, 5):
                    out = ops.concept_codes(x, c, 0.05, 0.3, iters)
                    yield f"concept_codes/{name}/V{V}i{iters}", dict(zip(("w", "resid2", "l1norm", "nnz", "delta", "kkt"), out))
            K = min(C, R)
            assign = torch.randint(0, K, (R,), generator=gen).cuda()
            yield f"kmeans_update/{name}", dict(zip(("c", "norm", "count"), ops.kmeans_update(x, assign, K, unit(2700 + i, K, D, dt))))
            for wtag, weight in (("", None), ("/weight", torch.rand(R, generator=gen).cuda())):
                mind = torch.full((R,), float("inf"), device="cuda")
                owner = torch.full((R,), -1, dtype=torch.int32, device="cuda")
                picks, radius, _ = ops.coreset_greedy(x, mind, owner, min(R, 6), first=R // 2, weight=weight)
                yield f"coreset_greedy/{name}{wtag}", {"picks": picks, "radius": radius, "mind": mind, "owner": owner}
            W, bias = rnd(2800 + i, C, D, scale=0.5).cuda(), rnd(2900 + i, C).cuda()
            rw = torch.rand(R, generator=gen).cuda()
            lse, loss, pred, logits = ops.probe_forward(x, W, bias, y, row_weight=rw, logits=True)
            yield f"probe_fwd/{name}", {"lse": lse, "loss": loss, "pred": pred, "logits": logits}
            dW, db, obj = ops.probe_backward(x, W, bias, y, lse, 1.0 / R, 1e-3, row_weight=rw, loss=loss)
            yield f"probe_bwd/{name}", {"dW": dW, "db": db, "objective": obj}
    for N in (1, 63, 65, 257, 3000):                                # tsne_merge_kernel and tsne_total_kernel: one block, a partial one, several
        yield f"tsne_repulsion/N{N}", dict(zip(("zrow", "rep", "z"), ops.tsne_repulsion(rnd(3000 + N, N, 2, scale=3.0).cuda())))


def row_inputs(C, seed):
    logits = rnd(seed, ROW_R, C, scale=3.0)
    logits[2] = 1.5                                                 # a row of ties: the first column is the argmax
    logits[6] = float("nan")                                        # a row without a maximum
    g = torch.Generator().manual_seed(seed + 1)
    row_class = torch.randint(-1, 4, (ROW_R,), generator=g).to(torch.int32)
    col_class = torch.randint(-1, 4, (C,), generator=g).to(torch.int32)
    labels = torch.randint(0, C, (ROW_R,), generator=g).to(torch.int32)
    labels[1] = -100
    return logits.cuda(), labels.cuda(), row_class.cuda(), col_class.cuda()


def row_cases():
    bias = torch.tensor([-0.75], device="cuda")
    for C in ROW_C:
        for grad in ("none", "f32", "alias", "bf16", "f16"):
            logits, labels, row_class, col_class = row_inputs(C, 600 + C)
            f = lambda dt=torch.float32: torch.zeros(ROW_R, device="cuda", dtype=dt)  # noqa: E731
            dl = {"none": None, "f32": torch.zeros_like(logits), "alias": logits, "bf16": torch.zeros_like(logits, dtype=torch.bfloat16),
                  "f16": torch.zeros_like(logits, dtype=torch.float16)}[grad]
            out = {"loss_row": f(), "pred": f(torch.int32)}
            if dl is not None:
                out.update(dlogits=dl, rowdot=f())
            ops.xent_rows(logits, labels, loss_row=out["loss_row"], pred=out["pred"], dlogits=dl, grad_scale=0.37, rowdot=out.get("rowdot"))
            yield f"xent_rows/C{C}/{grad}", out
            if grad in ("bf16", "f16"):
                continue
            logits, labels, row_class, col_class = row_inputs(C, 600 + C)
            dl = {"none": None, "f32": torch.zeros_like(logits), "alias": logits}[grad]
            out = {"loss_row": f(), "pred": f(torch.int32), "hit": f()}
            if dl is not None:
                out.update(dlogits=dl, rowdot=f())
            ops.xent_rows_classes(logits, row_class, col_class, loss_row=out["loss_row"], pred=out["pred"], hit=out["hit"], dlogits=dl,
                                  grad_scale=0.37, rowdot=out.get("rowdot"))
            yield f"xent_rows_classes/C{C}/{grad}", out
            logits, labels, row_class, col_class = row_inputs(C, 600 + C)
            dl = {"none": None, "f32": torch.zeros_like(logits), "alias": logits}[grad]
            out = {"loss_row": f(), "pred": f(torch.int32), "hit": f()}
            if dl is not None:
                out.update(dlogits=dl, rowdot=f(), rowsum=f())
            ops.sigmoid_rows(logits, row_class, col_class, bias, loss_row=out["loss_row"], pred=out["pred"], hit=out["hit"], dlogits=dl,
                             grad_scale=0.37, rowdot=out.get("rowdot"), rowsum=out.get("rowsum"))
            yield f"sigmoid_rows/C{C}/{grad}", out
            logits, labels, row_class, col_class = row_inputs(C, 600 + C)
            teacher = rnd(602 + C, ROW_R, C, scale=3.0).cuda()
            teacher[4] = logits[4]                                  # a teacher row equal to the student's: loss and gradient 0
            teacher[0, C // 2] = teacher[1, 0] = float("-inf")      # masked cells; [1, 0] is the first column lane 0 sees
            dl = {"none": None, "f32": torch.zeros_like(logits), "alias": logits}[grad]
            out = {"loss_row": f(), "pred": f(torch.int32), "agree": f()}
            if dl is not None:
                out.update(dlogits=dl, rowdot=f())
            ops.kl_rows(logits, padded(teacher, 8), loss_row=out["loss_row"], pred=out["pred"], agree=out["agree"], dlogits=dl,
                        grad_scale=0.37, rowdot=out.get("rowdot"))
            yield f"kl_rows/C{C}/{grad}", out


def select_cases():
    N = 3
    names = ("cos", "clip_score", "ref_score", "score", "order", "best")
    for K in (1, 5, 64):
        for E in (4, 512, 1024):
            img, txt, ref = rnd(700 + E, N, E).cuda(), rnd(710 + K + E, N * K, E).cuda(), rnd(720 + E, 4, E).cuda()
            if K > 1:
                txt[1] = txt[0]                                     # two candidates with equal scores: the lower k first
            lm = rnd(730 + K, N * K).cuda()
            lm_nan = lm.clone()
            lm_nan[N * K // 2] = float("nan")
            for tag, lm_mean in (("no_lm", None), ("lm", lm), ("lm_nan", lm_nan)):
                out = ops.caption_select(img, txt, K, lm_mean=lm_mean, ref=ref, ref_off=[0, 3, 3, 4], lm_weight=0.2)
                yield f"caption_select/K{K}/E{E}/{tag}", dict(zip(names, out))


def sample_cases():
    n = 4
    u = torch.tensor([0.0, 0.31, 0.77, 0.999], device="cuda")
    for V in (5, 4099, 50257):
        logits = rnd(800 + V, n, V, scale=2.0)
        logits[1, : min(V, 3)] = logits[1].max()                    # tied maxima
        logits = logits.cuda()
        for tag, kw in (("top_k", dict(top_k=4)), ("top_p", dict(top_p=0.8)), ("plain", {})):
            done = torch.tensor([0, 0, 1, 0], dtype=torch.int32, device="cuda")
            out = ops.sample_rows(logits, u, done, inv_temperature=1.25, stop_token=2, **kw)
            yield f"sample_rows/V{V}/{tag}", dict(zip(("token", "logprob", "n_kept", "kept_mass"), out), done=done)


def grid_cases():
    x = rnd(900, 9, 70).cuda()
    y, inv = torch.zeros_like(x), torch.zeros(9, device="cuda")
    ops.l2norm_fwd(x, y, inv)
    yield "l2norm_fwd/9x70", {"y": y, "inv_norm": inv}
    rows, L, D, V = 10, 5, 72, 11
    text = torch.randint(-1, V + 1, (rows,), generator=torch.Generator().manual_seed(901)).to(torch.int32).cuda()
    out = torch.zeros(rows, D, device="cuda")
    ops.text_embed(text, rnd(902, V, D).cuda(), rnd(903, L, D).cuda(), out, rows=rows, L=L)
    yield f"text_embed/{rows}x{D}", {"x": out}


def cases():
    """(name, {tensor name: tensor}) of every launch, in a fixed order"""
    for gen in (topk_cases, lm_cases, sweep_cases, pair_cases, row_cases, select_cases, sample_cases, grid_cases):
        yield from gen()


def raw(t):
    """the tensor's bytes on the host, as int8: every bit pattern (NaN payloads, 16-bit floats) compares as it is"""
    return t.detach().contiguous().cpu().view(torch.int8)


def main():
    ap = argparse.ArgumentParser()
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--out", help="run the cases and save every output tensor here")
    g.add_argument("--compare", help="run the cases and compare with the tensors saved here, byte by byte")
    args = ap.parse_args()
    saved = torch.load(args.compare) if args.compare else {}
    n_cases = n = 0
    for name, tensors in cases():
        for key, t in tensors.items():
            if t is None:
                continue
            now = (str(t.dtype), tuple(t.shape), raw(t))
            old = saved.get(f"{name}:{key}")
            if args.compare and not (old is not None and old[:2] == now[:2] and torch.equal(old[2], now[2])):
                print(f"DIFFERENT  {name}:{key}", flush=True)
                sys.exit(1)
            saved[f"{name}:{key}"] = now
            n += 1
        n_cases += 1
        print(f"{'same' if args.compare else 'run '}  {name}", flush=True)
    if args.compare:
        if n != len(saved):
            print(f"DIFFERENT  {len(saved)} tensors saved, {n} produced", flush=True)
            sys.exit(1)
        print(f"{n_cases} cases, {n} tensors byte-identical to {args.compare}")
    else:
        torch.save(saved, args.out)
        print(f"{n_cases} cases, {n} tensors saved to {args.out}")


if __name__ == "__main__":
    main()
