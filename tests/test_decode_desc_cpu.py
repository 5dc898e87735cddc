"""CPU: the descriptor fillers of the three decode entry points (ops.decode_step_desc, ops.beam_search_desc,
ops.beam_search_batch_desc) on small CPU tensors - no library is loaded and nothing is launched.  Every pointer field must be the
data_ptr() of the tensor it stands for, every stride and scalar its source, and each layout check must fire on one wrong input."""
import ctypes
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, D, HID, HEADS, BEAMS, MAX_LEN, V, POS, N_CAP = 2, 64, 128, 1, 3, 8, 40, 5, 2
DT = torch.bfloat16
ENTRIES = ("step", "beam", "batch")


def _setup(entry):
    from cclip_hip import ops
    rows = {"step": BEAMS, "beam": BEAMS, "batch": N_CAP * BEAMS}[entry]
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)                                   # noqa: E731
    blocks = [SimpleNamespace(**{n: f32(4) for n, _ in ops.BlockPtrs._fields_}) for _ in range(L)]
    blocks[1].b_qkv = None
    t = SimpleNamespace(ops=ops, rows=rows, blocks=blocks, arr=ops.block_ptr_array(blocks),
                        # a cache with room for more sequences than the step uses: ld_layer != rows * ld_seq
                        k=torch.zeros(L, rows + 1, MAX_LEN, D, dtype=DT)[:, :rows], v=torch.zeros(L, rows + 1, MAX_LEN, D, dtype=DT)[:, :rows],
                        scratch=torch.zeros(rows * (5 * D + HID), dtype=DT), lnf_w=f32(D), lnf_b=f32(D), wte16=torch.zeros(V, D, dtype=DT),
                        wte=f32(V, D), wpe=f32(MAX_LEN, D), logits=f32(rows, 48)[:, :V], x=f32(rows, D))
    if entry == "beam":
        t.st, t.first = ops.BeamState(BEAMS, MAX_LEN, 6, "cpu"), f32(V)
    if entry == "batch":
        t.st, t.first = ops.BeamBatchState(N_CAP, BEAMS, MAX_LEN, 6, "cpu"), f32(N_CAP, V)
    return t


def _fill(entry, t, **over):
    a = {**vars(t), **over}
    kw = dict(heads=HEADS, hidden=HID, act=t.ops.ACT_GELU_NEW, lnf_w=a["lnf_w"], lnf_b=a["lnf_b"], wte16=a["wte16"])
    if entry == "step":
        return t.ops.decode_step_desc(t.arr, L, a["x"], a["k"], a["v"], POS, a["scratch"], linear_layout=True, logits=a["logits"], **kw)
    kw.update(wte_f32=a["wte"], wpe_f32=a["wpe"], temperature=0.5, stop_token=7, first_logits=a["first"], grid_cap=3)
    if entry == "beam":
        return t.ops.beam_search_desc(t.arr, L, t.st, a["k"], a["v"], POS, a["scratch"], 4, logits=a["logits"], **kw)
    return t.ops.beam_search_batch_desc(t.arr, L, t.st, a["k"], a["v"], POS, a["scratch"], 4, **kw)


def _check_step(s, t, x, linear_layout, logits):
    assert ctypes.addressof(s.blocks.contents) == ctypes.addressof(t.arr)
    for i, blk in enumerate(t.blocks):
        for n, _ in t.ops.BlockPtrs._fields_:
            w = getattr(blk, n)
            assert (getattr(t.arr[i], n) or 0) == (0 if w is None else w.data_ptr()), (i, n)
    want = dict(n_layer=L, n_seq=t.rows, width=D, heads=HEADS, hidden=HID, act=t.ops.ACT_GELU_NEW, linear_layout=int(linear_layout),
                pos=POS, x=x.data_ptr(), kcache=t.k.data_ptr(), vcache=t.v.data_ptr(), ld_layer=(t.rows + 1) * MAX_LEN * D,
                ld_seq=MAX_LEN * D, scratch16=t.scratch.data_ptr(), lnf_w=t.lnf_w.data_ptr(), lnf_b=t.lnf_b.data_ptr(),
                wte16=t.wte16.data_ptr(), vocab=V, logits=logits.data_ptr() if logits is not None else None,
                ld_logits=48 if logits is not None else 0)
    assert {n: getattr(s, n) for n in want} == want
    assert set(want) | {"blocks"} == {f[0] for f in t.ops.DecodeDesc._fields_}


def _check_beam(d, t, own):
    st = t.st
    assert st.x.shape == (t.rows, D) and st.x.dtype == torch.float32
    _check_step(d.step, t, st.x, False, t.logits if "first" in own else None)
    want = dict(n_steps=4, stop_token=7, ld_tokens=6, max_len=MAX_LEN, grid_cap=3, temperature=0.5, first_logits=t.first.data_ptr(),
                wte_f32=t.wte.data_ptr(), wpe_f32=t.wpe.data_ptr(), **{n: getattr(st, n).data_ptr() for n in t.ops._BEAM_BUFFERS}, **own)
    assert {n: getattr(d, n) for n in want} == want
    assert set(want) | {"step"} == {f[0] for f in type(d)._fields_}
    assert len({getattr(d, n) for n in t.ops._BEAM_BUFFERS}) == len(t.ops._BEAM_BUFFERS)


def test_step_descriptor_carries_its_tensors():
    t = _setup("step")
    _check_step(_fill("step", t), t, t.x, True, t.logits)


def test_one_caption_descriptor_carries_state_and_tensors():
    t = _setup("beam")
    assert t.st.x is None and t.st.slot_of.shape == (MAX_LEN, 8)
    _check_beam(_fill("beam", t), t, dict(first=1))
    x = t.st.x
    d = _fill("beam", t, first=None)                         # a continued search: no first selection, the same x rows
    assert d.first == 0 and d.first_logits is None and t.st.x is x and d.step.x == x.data_ptr()


def test_batched_descriptor_carries_state_and_tensors():
    t = _setup("batch")
    assert t.st.x is None and t.st.slot_of.shape == (N_CAP, MAX_LEN, 8) and t.st.cap_state.shape == (N_CAP, 8)
    _check_beam(_fill("batch", t), t, dict(n_cap=N_CAP, beams=BEAMS, cap_state=t.st.cap_state.data_ptr()))


@pytest.mark.parametrize("entry", ENTRIES)
def test_layout_checks_fire(entry):
    t = _setup(entry)
    _fill(entry, t)                                                                       # the inputs are right as they stand
    wide = torch.zeros(L, t.rows, MAX_LEN, 2 * D, dtype=DT)[..., :D]                       # stride(2) = 2 * width
    with pytest.raises(AssertionError):
        _fill(entry, t, k=wide, v=wide)
    with pytest.raises(AssertionError):
        _fill(entry, t, scratch=t.scratch[:-1])
    if entry != "step":                                                                   # the beam-only checks
        with pytest.raises(AssertionError):
            _fill(entry, t, wte=t.wte.half())
        longer = torch.zeros(L, t.rows, MAX_LEN + 1, D, dtype=DT)
        with pytest.raises(AssertionError):
            _fill(entry, t, k=longer, v=longer)
