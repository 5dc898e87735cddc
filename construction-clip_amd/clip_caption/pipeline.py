"""One call from image to caption: what the reference serves as `/predict` (/root/reference/application.py:80-108, root
predict.py:62-76, `predict()` of CLIP_prefix_caption/test.py:516-549) - encode the image, two zero-shot heads (caption type,
violation type), the attribute string they select as decoder prompt, the prefix projection, beam search - with the device
stage enqueued back to back and nothing read by the host in between.

The attribute string `f"{caption_type} {violation_type} "` has only len(caption_types) * len(violation_types) = 18 values.  All
of them are tokenised ONCE, when the Captioner is built, into an id table on the device; which row an image gets is an
index the device computes from its feature vector (cclip_caption_prompt: both heads' softmax, arg-max and the table row in one
launch for all N images).  The reference's per-image `.cpu()` / arg-max / `tokenizer.encode` / host-built id tensor / `wte` /
`torch.cat` between encode_image and the decoder are gone; `cclip_caption_embed` writes the decoder's input rows from the
projected prefix and the selected ids.

Labels: like `extract_embeddings` (parse_coco.py:47,54) and test.py:527,532 a head reports `caption_types.values()` (現況 / 缺失)
and the entries of `violation_types`; application.py's English keys are only the CLIP prompts.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import torch

from cclip_hip import ops

from .data import CAPTION_TYPES, VIOLATION_TYPES
from .generate import _beam_outputs, _beam_rows, _replay_attention, generate2_batch, generate_beam_batch, generate_sample_batch


def attribute_strings(caption_labels: Sequence[str], violation_labels: Sequence[str]) -> List[str]:
    """every attribute string test.py:534 can form, caption type slowest (row i * len(violation_labels) + j)"""
    return [f"{c} {v} " for c in caption_labels for v in violation_labels]


def build_attribute_table(tokenizer, caption_labels: Sequence[str], violation_labels: Sequence[str],
                          attribute_length: int) -> torch.Tensor:
    """int32 [len(caption_labels) * len(violation_labels), attribute_length]: `tokenizer.encode` of every attribute string, right
    padded with id 0 (test.py:536-538).  A string that needs more ids than attribute_length raises ValueError (the reference
    fails there with a negative pad size)."""
    strings = attribute_strings(caption_labels, violation_labels)
    table = torch.zeros(len(strings), attribute_length, dtype=torch.int32)
    for r, s in enumerate(strings):
        enc = list(tokenizer.encode(s))
        if len(enc) > attribute_length:
            raise ValueError(f"attribute {s!r} needs {len(enc)} token ids, attribute_length is {attribute_length}")
        table[r, :len(enc)] = torch.tensor(enc, dtype=torch.int32)
    return table


def _check_best_of(best_of, return_attention: bool) -> None:
    if int(best_of) != best_of or best_of < 0:
        raise ValueError(f"best_of must be an integer >= 0 (0 = beam search), got {best_of}")
    if best_of and best_of > ops.CAPTION_SELECT_MAX_K:
        raise NotImplementedError(f"best_of = {best_of}; the selection kernel ranks at most {ops.CAPTION_SELECT_MAX_K} candidates")
    if best_of and return_attention:
        raise NotImplementedError("return_attention is not available with best_of")


class PendingCaptions:
    """What Captioner.submit returns: the device work is enqueued; result() reads it back and decodes the text."""

    def __init__(self, cap: "Captioner", n: int, probs, index, ids, greedy: bool, pending=None, eager=None, proj=None, select=None):
        self._cap, self._n, self._probs, self._index, self._ids = cap, n, probs, index, ids
        self._greedy, self._pending, self._eager = greedy, pending, eager
        self._proj = proj                                                 # the projected prefixes, kept for return_attention
        self._select = select                                             # best_of: what Captioner._clip_select left on the device
        self._done = None

    def _attention(self, per):
        """the best beam's rows [H, n, S0 + n - 1] of the last layer for every image: one replay forward for all of them"""
        cap = self._cap
        model = cap.caption_model
        emb = torch.cat((self._proj.view(self._n, cap.prefix_length, -1), model.gpt.transformer.wte(self._ids.long())), dim=1)
        if self._greedy:
            gen = [rows[0] for rows in per]
        else:                                                              # scores are length-normalised: _beam_outputs' order
            gen = [_beam_rows(tk, ln, 0)[int(sc.argsort(descending=True)[0])] for tk, ln, sc in per]
        return _replay_attention(model, [emb[i] for i in range(self._n)], gen, -1)

    def result(self, return_tokens: bool = False):
        if self._done is None:
            cap, tok = self._cap, self._cap.tokenizer
            if self._pending is not None:                                 # the read-back of the batched launches
                tokens, lengths, scores, n_sel = cap.caption_model.beam_batch_collect(self._pending)
                self._pending = None
                texts, per = [], []
                for i in range(self._n):
                    rows = tokens[i, :, :int(n_sel[i])]
                    if self._greedy:                                       # generate2_batch's decode of the one-beam row
                        texts.append(tok.decode(list(rows.squeeze(0).cpu().numpy())))
                        per.append(rows)
                    else:                                                  # generate_beam_batch's: best beam first
                        t, tk, ln, sc = _beam_outputs(tok, rows, lengths[i], scores[i], True)
                        texts.append(t[0])
                        per.append((tk, ln, sc))
            else:
                texts, per = self._eager
            probs, index, ids = self._probs.cpu(), self._index.cpu(), self._ids.cpu()
            k0 = cap.head_start[1]
            records = []
            for i in range(self._n):
                c, v = int(index[i, 0]), int(index[i, 1])
                records.append({"caption_type": cap.caption_labels[c], "violation_type": cap.violation_labels[v],
                                "attribute": cap.attributes[c * len(cap.violation_labels) + v], "prediction": texts[i],
                                "type_probs": probs[i, :k0].tolist(), "violation_probs": probs[i, k0:].tolist()})
            if self._proj is not None:
                for rec, att in zip(records, self._attention(per)):
                    rec["attention"] = att
            extras = {"ids": ids, "index": index, "tokens": per}
            if self._select is not None:                                  # texts[i] is still unset: the selection names it
                sel = self._select
                K, cand = sel["K"], sel["texts"]
                cos, cs, lm, order = (sel[k].cpu().reshape(self._n, K).tolist() for k in ("cos", "clip_score", "lm_mean", "order"))
                for i, rec in enumerate(records):
                    rec["candidates"] = [{"text": cand[i * K + k], "cos": cos[i][k], "clip_score": cs[i][k], "lm_logprob": lm[i][k]}
                                         for k in order[i]]
                    rec["prediction"] = rec["candidates"][0]["text"]
                    rec["clip_score"] = rec["candidates"][0]["clip_score"]
                extras.update(text_features=sel["text_features"], order=sel["order"])
            self._done = (records, extras)
        return self._done if return_tokens else self._done[0]


class Captioner:
    """Captioner(clip_model, caption_model, tokenizer).describe(images) -> one record per image:
    {"caption_type", "violation_type", "attribute", "prediction", "type_probs", "violation_probs"}.

    clip_tokenize turns the prompt strings into CLIP token rows (default clip.tokenize); the prompts are
    `caption_types.keys()` and `violation_types`, the reported labels `caption_types.values()` and `violation_types` (as
    extract_embeddings / test.py do; application.py reports the keys).  caption_model may be None for a Captioner that is only
    asked to `embed`.  preprocess (default clip.DevicePreprocess at the model's
    resolution) is applied to PIL images / uint8 HWC arrays; float tensors [N, 3, R, R] are taken as preprocessed."""

    def __init__(self, clip_model, caption_model, tokenizer, clip_tokenize: Optional[Callable] = None,
                 caption_types: Optional[Dict[str, str]] = None, violation_types: Optional[Sequence[str]] = None,
                 prefix_length: int = 20, attribute_length: int = 20, preprocess: Optional[Callable] = None):
        if clip_tokenize is None:
            from clip import tokenize as clip_tokenize
        caption_types = dict(CAPTION_TYPES if caption_types is None else caption_types)
        violation_types = list(VIOLATION_TYPES if violation_types is None else violation_types)
        self.clip_model, self.caption_model, self.tokenizer = clip_model, caption_model, tokenizer
        self.clip_tokenize = clip_tokenize                                 # explain() tokenises the generated captions with it
        self.prefix_length, self.attribute_length = prefix_length, attribute_length
        self.caption_labels, self.violation_labels = list(caption_types.values()), violation_types
        self.attributes = attribute_strings(self.caption_labels, self.violation_labels)
        self.device = clip_model.logit_scale.device
        self._preprocess = preprocess
        with torch.no_grad():                                              # the prompts of both heads, encoded once
            heads = [clip_model.encode_text(clip_tokenize(p).to(self.device)).float()
                     for p in (list(caption_types.keys()), violation_types)]
        self.prompts = torch.cat(heads).contiguous()
        self.head_start = (0, heads[0].shape[0], heads[0].shape[0] + heads[1].shape[0])
        self.table = build_attribute_table(tokenizer, self.caption_labels, self.violation_labels, attribute_length).to(self.device)

    # ---- input ----
    def _images(self, images) -> torch.Tensor:
        if isinstance(images, torch.Tensor) and images.is_floating_point():
            if images.dim() != 4 or images.shape[1] != 3:
                raise ValueError(f"preprocessed images must be [N, 3, R, R], got {tuple(images.shape)}")
            return images.to(self.device, non_blocking=True)
        if self._preprocess is None:
            from clip import DevicePreprocess
            self._preprocess = DevicePreprocess(self.clip_model.visual.input_resolution, self.device)
        return torch.stack([self._preprocess(im).to(self.device) for im in images])

    # ---- device stage ----
    def _classify(self, feat: torch.Tensor):
        N = feat.shape[0]
        probs = torch.empty(N, self.prompts.shape[0], device=feat.device, dtype=torch.float32)
        index = torch.empty(N, 2, device=feat.device, dtype=torch.int32)
        ids = torch.empty(N, self.attribute_length, device=feat.device, dtype=torch.int32)
        scale = self.clip_model.logit_scale.detach().float().reshape(1)
        ops.caption_prompt(feat, self.prompts, self.head_start, scale, self.table, probs, index, ids)
        return probs, index, ids

    @torch.no_grad()
    def embed(self, images, batch_size: int = 256):
        """(features [N, E] fp32, index int32 [N, 2], ids int32 [N, attribute_length]) on the device, without decoding: what
        parse_coco.py:38-56 computes per annotation (the embedding, the two zero-shot arg-maxes, the attribute's ids)."""
        images = self._images(images)
        feat = torch.cat([self.clip_model.encode_image(images[s:s + batch_size]).float() for s in range(0, images.shape[0], batch_size)])
        _, index, ids = self._classify(feat.contiguous())
        return feat, index, ids

    def _features_one_by_one(self, images: torch.Tensor) -> torch.Tensor:
        # image by image, like the decoder's prefills: the tiled GEMMs choose tiles / splits by row count, so a batched tower
        # would make an image's features - and through the 16-bit prefix its tokens - depend on the images around it
        return torch.cat([self.clip_model.encode_image(images[i:i + 1]).float() for i in range(images.shape[0])]).contiguous()

    def _project(self, feat: torch.Tensor) -> torch.Tensor:
        N = feat.shape[0]
        return torch.cat([self.caption_model.clip_project(feat[i:i + 1]).reshape(1, -1) for i in range(N)]).contiguous()

    def _clip_select(self, images, feat, per, K: int, lm_weight: float, score_model):
        """CLIP's choice among the K draws of every image.  per: generate_sample_batch's N tuples (texts, tokens [K, steps],
        lengths, sum_logprob) in draw order.  Returns what PendingCaptions.result needs, everything but the texts on the device."""
        from clip.score import encode_distinct_texts
        tok = self.tokenizer
        texts, lm = [], []
        for _, tokens, lengths, total in per:
            rows, lens = tokens.cpu().numpy(), lengths.tolist()
            texts += [tok.decode(list(rows[k][:lens[k]])) for k in range(K)]          # draw order (the tuple's texts are sorted)
            lm.append(total / lengths)
        scorer = self.clip_model if score_model is None else score_model
        if scorer is not self.clip_model:                                  # the cosine needs both sides from one model
            was = scorer.training
            feat = torch.cat([scorer.encode_image(images[i:i + 1]).float() for i in range(images.shape[0])]).contiguous()
        text_features = encode_distinct_texts(scorer, self._caption_tokens(texts))
        if scorer is not self.clip_model and scorer.training != was:
            scorer.train(was)
        lm_mean = torch.cat(lm).float().contiguous()
        cos, cs, _, score, order, best = ops.caption_select(feat, text_features, K, lm_mean=lm_mean, lm_weight=float(lm_weight))
        return {"K": K, "texts": texts, "lm_mean": lm_mean, "cos": cos, "clip_score": cs, "score": score, "order": order, "best": best,
                "text_features": text_features}

    @torch.no_grad()
    def submit(self, images: torch.Tensor, beam_size: int = 3, entry_length: int = 100, temperature: float = 0.5,
               stop_token: int = 102, greedy: bool = False, top_p: float = 0.8, return_attention: bool = False, best_of: int = 0,
               lm_weight: float = 0.0, generator=None, uniforms=None, top_k: int = 0, score_model=None) -> PendingCaptions:
        """Enqueue the whole device stage for preprocessed images [N, 3, R, R] - encode_image, the zero-shot heads and attribute
        ids, clip_project, the decoder's input rows, the prefills and the batched beam launches - and return without waiting
        for the device; `.result()` reads back and decodes.  Where the batched kernel does not apply
        (ClipCaptionModel.beam_batch_native_ok) the work is done here, through generate_beam_batch / generate2_batch.
        return_attention: every record of `.result()` also gets "attention", the best beam's last-layer rows
        [H, n, S0 + n - 1] on the device (S0 = prefix_length + attribute_length; generate_beam's return_attention).
        best_of = K >= 1: instead of the beam search, K captions per image are DRAWN (generate_sample_batch with top_p, top_k,
        temperature; `generator` or `uniforms` [entry_length, N * K] fix the draw) and CLIP picks among them: the N * K texts
        go through score_model's text tower (default: the Captioner's CLIP model; distinct texts once) and one
        cclip_caption_select launch ranks them by cos(image, text) + lm_weight * (mean token log-probability).  The sampler's
        loop and the decoding of the candidates to text wait for the device, so this form returns after the selection is
        enqueued rather than at once.  beam_size and greedy are not used then."""
        model = self.caption_model
        images = self._images(images)
        N = images.shape[0]
        if N < 1:
            raise ValueError("need at least one image")
        _check_best_of(best_of, return_attention)
        P, A = self.prefix_length, self.attribute_length
        beams = 1 if greedy else beam_size
        ok = getattr(model, "beam_batch_native_ok", None)
        native = ok is not None and (top_p > 0 or not greedy) and ok(beams, P + A, entry_length)
        was_training = getattr(model, "training", None)
        try:
            feat = self._features_one_by_one(images)
            probs, index, ids = self._classify(feat)
            proj = self._project(feat)                                     # test.py:521,540: on the fp32 features
            if best_of:
                emb = torch.cat((proj.view(N, P, -1), model.gpt.transformer.wte(ids.long())), dim=1)
                per = generate_sample_batch(model, self.tokenizer, emb, num_samples=int(best_of), entry_length=entry_length, top_p=top_p,
                                            top_k=top_k, temperature=temperature, stop_token=stop_token, generator=generator,
                                            uniforms=uniforms, return_tokens=True)
                select = self._clip_select(images, feat, per, int(best_of), lm_weight, score_model)
                return PendingCaptions(self, N, probs, index, ids, greedy, eager=([None] * N, per), select=select)
            if native:
                D = proj.shape[1] // P
                x = torch.empty(N * (P + A), D, device=feat.device, dtype=torch.float32)
                tr = model.gpt.transformer
                ops.caption_embed(proj, ids, tr.wte.weight.data, tr.wpe.weight.data, x, B=N, P=P, Lt=A)
                pending = model.beam_batch_enqueue(x.view(N, P + A, D), beams, entry_length, temperature, stop_token,
                                                   positions_added=True)
                return PendingCaptions(self, N, probs, index, ids, greedy, pending=pending, proj=proj if return_attention else None)
            emb = torch.cat((proj.view(N, P, -1), model.gpt.transformer.wte(ids.long())), dim=1)      # test.py:540-542
            if greedy:
                eager = generate2_batch(model, self.tokenizer, emb, entry_length=entry_length, top_p=top_p, temperature=temperature,
                                        stop_token=stop_token, return_tokens=True)
            else:
                texts, per = generate_beam_batch(model, self.tokenizer, emb, beam_size=beam_size, entry_length=entry_length,
                                                 temperature=temperature, stop_token=stop_token, return_tokens=True)
                eager = ([t[0] for t in texts], per)
            return PendingCaptions(self, N, probs, index, ids, greedy, eager=eager, proj=proj if return_attention else None)
        finally:
            if was_training is not None and model.training != was_training:   # (generate_* switch the model to eval)
                model.train(was_training)

    def describe(self, images, beam_size: int = 3, entry_length: int = 100, temperature: float = 0.5, stop_token: int = 102,
                 greedy: bool = False, top_p: float = 0.8, return_tokens: bool = False, return_attention: bool = False,
                 best_of: int = 0, lm_weight: float = 0.0, generator=None, uniforms=None, top_k: int = 0, score_model=None):
        """The records of `images` (a preprocessed float tensor [N, 3, R, R], or a sequence of PIL images / uint8 HWC arrays).
        More images than one batched launch holds (64 // beams) go in chunks of that size; the next chunk is enqueued before
        the previous one is read back.  return_tokens: also {"ids" [N, A], "index" [N, 2], "tokens": per caption what
        generate_beam_batch (generate2_batch with greedy) returns with return_tokens}.  return_attention: as for submit.
        best_of = K >= 1 (as for submit): K captions are drawn per image and the one CLIP scores highest becomes "prediction";
        every record gains "clip_score" (the CLIPScore 2.5 max(cos, 0) of the prediction) and "candidates", K dicts {"text",
        "cos", "clip_score", "lm_logprob"} best first; "tokens" of the extras holds generate_sample_batch's tuples, and the
        extras gain "text_features" (fp32 [N * K, E], the rows the selection kernel saw, draw order) and "order" (int32 [N, K]).
        uniforms: [entry_length, N * K], column i * K + j = draw j of image i.  Chunks hold 64 // K images."""
        _check_best_of(best_of, return_attention)
        images = self._images(images)
        K = int(best_of)
        per = max(1, ops.BEAM_BATCH_MAX_ROWS // (K if K else 1 if greedy else max(1, beam_size)))
        kw = dict(beam_size=beam_size, entry_length=entry_length, temperature=temperature, stop_token=stop_token, greedy=greedy,
                  top_p=top_p, return_attention=return_attention)
        if best_of:
            kw.update(best_of=best_of, lm_weight=lm_weight, generator=generator, top_k=top_k, score_model=score_model)
            if uniforms is not None and tuple(uniforms.shape) != (entry_length, images.shape[0] * K):
                raise ValueError(f"uniforms must be [{entry_length}, {images.shape[0] * K}] (entry_length, N * best_of), "
                                 f"got {tuple(uniforms.shape)}")
        records, extras, prev = [], [], None
        for s in range(0, images.shape[0], per):
            if K and uniforms is not None:
                kw["uniforms"] = uniforms[:, s * K:(s + per) * K]
            nxt = self.submit(images[s:s + per], **kw)
            if prev is not None:
                r, e = prev.result(True)
                records += r
                extras.append(e)
            prev = nxt
        if prev is None:
            raise ValueError("need at least one image")
        r, e = prev.result(True)
        records += r
        extras.append(e)
        if not return_tokens:
            return records
        out = {"ids": torch.cat([e["ids"] for e in extras]), "index": torch.cat([e["index"] for e in extras]),
               "tokens": [t for e in extras for t in e["tokens"]]}
        if K:
            out.update(text_features=torch.cat([e["text_features"] for e in extras]), order=torch.cat([e["order"] for e in extras]))
        return records, out

    def _caption_tokens(self, texts: List[str]) -> torch.Tensor:
        """CLIP token rows of generated captions; an over-long caption is cut where clip_tokenize can do that (`truncate`)"""
        import inspect
        try:
            cut = "truncate" in inspect.signature(self.clip_tokenize).parameters
        except (TypeError, ValueError):
            cut = False
        return (self.clip_tokenize(texts, truncate=True) if cut else self.clip_tokenize(texts)).to(self.device)

    def explain(self, images, size: int = 224, relevance_model=None, start_layer: int = -1, start_layer_text: int = -1, lut=None,
                **describe_kwargs):
        """Caption plus why, for a batch (the reference's root predict.py:57-86 per photo): `describe(images)`, the N predictions
        tokenised with clip_tokenize, `clip.interpret_rows` of every (image, own caption) pair on relevance_model (default: the
        Captioner's CLIP model; the reference loads a second checkpoint for this, predict.py:46,50), then `clip.relevance_overlay`
        and `clip.text_row_scores`.  Returns describe's records, each extended with "overlay" (uint8 [size, size, 3] numpy, RGB),
        "image_relevance" (fp32 [patches]), "token_scores" (fp32 over the caption's tokens 1 .. EOT-1, summing to 1) and
        "clip_tokens" (the caption's CLIP token row), the last three on the device.  The overlays of the whole batch come back
        in one copy.  size / lut: as for clip.relevance_overlay; describe_kwargs go to describe (with return_tokens=True the
        result is (records, extras), as there; with best_of=K the caption explained is the one CLIP selected, and
        score_model=relevance_model scores the candidates on the model that explains them)."""
        import clip
        images = self._images(images)
        res = self.describe(images, **describe_kwargs)
        records = res[0] if describe_kwargs.get("return_tokens") else res
        tokens = self._caption_tokens([r["prediction"] for r in records])
        model = self.clip_model if relevance_model is None else relevance_model
        r_text, r_image = clip.interpret_rows(images, tokens, model, device=self.device, start_layer=start_layer,
                                              start_layer_text=start_layer_text)
        overlays = clip.relevance_overlay(r_image.contiguous(), images.float().contiguous(), size=size, lut=lut).cpu().numpy()
        scores = clip.text_row_scores(r_text, tokens)
        for i, rec in enumerate(records):
            rec.update(overlay=overlays[i], image_relevance=r_image[i], token_scores=scores[i], clip_tokens=tokens[i])
        return res
