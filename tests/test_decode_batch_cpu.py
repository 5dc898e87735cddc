"""CPU: the batched beam-search entry points are declared in include/cclip_hip.h, the ctypes descriptors of the three decode
entry points match their C structs field for field, and generate_beam_batch / generate2_batch refuse embeddings that are not [N, S, D] with N >= 1."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _header():
    hdr = open(os.path.join(ROOT, "include", "cclip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_batch_entry_points():
    hdr = _header()
    for name in ("cclip_gpt2_beam_search_batch", "cclip_gpt2_beam_search_batch_f16"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*const\s+cclip_beam_batch_desc\s*\*\s*\w+\s*,\s*hipStream_t", hdr), name


def _c_fields(hdr, struct):
    body = re.search(r"typedef\s+struct\s+" + struct + r"\s*\{(.*?)\}\s*" + struct + r"\s*;", hdr, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"((?:const\s+)?\w+)\s*(.*)$", decl, flags=re.S)
        ctype, rest = m.group(1).replace("const ", ""), m.group(2)
        for name in (n.strip() for n in rest.split(",")):
            ptr = name.startswith("*")
            fields.append((name.lstrip("* "), "ptr" if ptr else ctype))
    return fields


def _check_struct(struct, cls_name):
    from cclip_hip import ops
    cls = getattr(ops, cls_name)
    fields = _c_fields(_header(), struct)
    kinds = {"int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "ptr": ctypes.c_void_p,
             "cclip_decode_desc": ops.DecodeDesc}
    ref = type("Ref", (ctypes.Structure,), {"_fields_": [(n, kinds[k]) for n, k in fields]})
    got = [f[0] for f in cls._fields_]
    assert got == [n for n, _ in fields]
    for n, _ in fields:
        assert getattr(cls, n).offset == getattr(ref, n).offset, n
        assert getattr(cls, n).size == getattr(ref, n).size, n
    assert ctypes.sizeof(cls) == ctypes.sizeof(ref)


def test_ctypes_descriptor_matches_header_struct():
    from cclip_hip import ops
    _check_struct("cclip_beam_batch_desc", "BeamBatchDesc")
    assert ops.BEAM_BATCH_MAX_ROWS == 64


@pytest.mark.parametrize("struct, cls_name", [("cclip_beam_desc", "BeamDesc"), ("cclip_decode_desc", "DecodeDesc"),
                                              ("cclip_block_ptrs", "BlockPtrs")])
def test_step_and_one_caption_descriptors_match_header_structs(struct, cls_name):
    _check_struct(struct, cls_name)


@pytest.mark.parametrize("bad", [torch.zeros(8, 16), torch.zeros(0, 8, 16), torch.zeros(1, 2, 8, 16)])
def test_batch_generators_reject_bad_embeds(bad):
    from clip_caption import generate2_batch, generate_beam_batch
    with pytest.raises(ValueError, match=r"\[N, S, D\]"):
        generate_beam_batch(object(), None, bad)
    with pytest.raises(ValueError, match=r"\[N, S, D\]"):
        generate2_batch(object(), None, bad)
