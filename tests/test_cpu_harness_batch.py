"""The batched directory harness's host side: the batch plan, the CLI flag, the
signatures and the header declarations.  No device."""
import inspect
import os
import re

import pytest

from conftest import REPO


def _plan(shapes, bs):
    from enhancers.simple_enhance import plan_batches
    return plan_batches(shapes, bs)


def _check_partition(shapes, bs, batches):
    assert sorted(i for b in batches for i in b) == list(range(len(shapes)))
    for b in batches:
        assert 1 <= len(b) <= bs
        assert len({tuple(shapes[i]) for i in b}) == 1
        assert b == sorted(b)


def test_plan_is_a_partition_by_shape():
    shapes = [(64, 96), (96, 64), (64, 96), (32, 32), (64, 96), (96, 64), (64, 96), (64, 96), (64, 96)]
    for bs in (1, 2, 3, 4, 100):
        batches = _plan(shapes, bs)
        _check_partition(shapes, bs, batches)
        assert batches == _plan(list(shapes), bs)  # deterministic
    # full buckets leave when they fill, the rest at the end in order of their first index
    assert _plan(shapes, 4) == [[0, 2, 4, 6], [1, 5], [3], [7, 8]]
    assert _plan(shapes, 1) == [[i] for i in range(len(shapes))]


def test_plan_keeps_at_most_eight_buckets_open():
    from enhancers.simple_enhance import MAX_OPEN_BUCKETS
    assert MAX_OPEN_BUCKETS == 8
    shapes = [(8 * (k + 1), 8) for k in range(10)]
    batches = _plan(shapes, 4)
    _check_partition(shapes, 4, batches)
    # shape 8 pushes out bucket [0], shape 9 bucket [1]; the other eight leave at the end in order
    assert batches == [[k] for k in range(10)]
    # the pushed-out bucket is the one with the oldest first index, emitted short; its shape may reopen
    shapes = [(8, 8), (16, 8), (8, 8)] + [(8 * k, 8) for k in range(3, 10)] + [(8, 8), (16, 8)]
    batches = _plan(shapes, 4)
    _check_partition(shapes, 4, batches)
    assert batches[0] == [0, 2]       # 9 shapes seen at index 9: (8, 8)'s bucket leaves with two entries
    assert batches[1] == [1]          # index 10 reopens (8, 8): (16, 8)'s bucket is now the oldest
    assert batches[2:] == [[3], [4], [5], [6], [7], [8], [9], [10], [11]]


def test_plan_edge_cases():
    assert _plan([], 4) == []
    for bad in (0, -1):
        with pytest.raises(ValueError):
            _plan([(8, 8)], bad)


def test_infer_batch_flag_and_signatures():
    import main as cli
    from enhancers import simple_enhance as se
    p = cli.build_parser()
    assert p.parse_args([]).infer_batch == 1
    assert p.parse_args(["--infer_batch", "8"]).infer_batch == 8
    sig = inspect.signature(se.enhance_batch_images)
    assert sig.parameters["batch_size"].default == 1
    assert sig.parameters["decode_threads"].default == 4
    assert callable(se.run_batched) and callable(se.plan_batches)


def test_header_declares_the_batched_entry_points():
    src = open(os.path.join(REPO, "include", "upr.h")).read()
    assert re.search(r"\}\s*upr_letterbox_rec\s*;", src)
    assert re.search(r"\bint\s+upr_letterbox_batch\s*\(\s*const\s+upr_letterbox_rec\s*\*", src)
    assert re.search(r"\bint\s+upr_panels_u8\s*\(", src)
    # the ctypes record mirrors the C struct: three pointers, six int32
    import ctypes
    from upr import _lib as L
    assert ctypes.sizeof(L.UprLetterboxRec) == 3 * ctypes.sizeof(ctypes.c_void_p) + 6 * 4
    assert [f[0] for f in L.UprLetterboxRec._fields_] == ["src", "xtab", "ytab", "H", "W", "top", "left", "nh", "nw"]


def test_batched_entry_points_refuse_bad_arguments_without_a_device():
    from upr import _lib as L
    lib = L.lib()
    one = 16  # any non-NULL value: refused before it is used
    assert lib.upr_letterbox_batch(None, 1, 8, 8, 0, one, L.UPR_F32, None) == L.UPR_ERR_ARG
    assert lib.upr_letterbox_batch(one, 1, 8, 8, 0, None, L.UPR_F32, None) == L.UPR_ERR_ARG
    assert lib.upr_letterbox_batch(one, 0, 8, 8, 0, one, L.UPR_F32, None) == L.UPR_ERR_ARG
    assert lib.upr_letterbox_batch(one, 1, 8, 8, 0, one, 7, None) == L.UPR_ERR_ARG
    assert lib.upr_panels_u8(None, one, None, 1, 8, 8, L.UPR_F32, one, None, None, 0, None) == L.UPR_ERR_ARG
    assert lib.upr_panels_u8(one, one, None, 0, 8, 8, L.UPR_F32, one, None, None, 0, None) == L.UPR_ERR_ARG
    assert lib.upr_panels_u8(one, one, None, 1, 8, 8, 7, one, None, None, 0, None) == L.UPR_ERR_ARG
    assert lib.upr_panels_u8(one, one, None, 1, 8, 8, L.UPR_F32, one, None, one, 3, None) == L.UPR_ERR_ARG  # no illu
    assert lib.upr_panels_u8(one, one, None, 1, 8, 8, L.UPR_F32, one, one, None, 0, None) == L.UPR_ERR_ARG
    assert lib.upr_panels_u8(one, one, one, 1, 8, 8, L.UPR_F32, one, None, one, 4, None) == L.UPR_ERR_ARG
