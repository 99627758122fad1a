"""libupr.so loads on a GPU-less host and exports exactly the C ABI declared in
include/upr.h; host-side tables agree with the numpy oracle.  No device calls."""
import ctypes
import os
import re

import numpy as np

from conftest import REPO
from oracle import cv_u8
from upr import _lib as L
from upr import runtime


def header_functions(headers=("upr.h", "upr_train.h")):
    names = set()
    for h in headers:
        src = open(os.path.join(REPO, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(upr_[a-z0-9_]+)\s*\(", src))
    return sorted(names)


def test_library_builds_and_loads():
    assert os.path.exists(L.LIB_PATH), "run __graft_entry__.build() first"
    assert L.lib() is not None


def test_exports_every_header_symbol():
    names = header_functions()
    assert len(names) >= 60
    cdll = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(cdll, n), f"{n} declared in include/upr.h but not exported"
    # the ctypes binding covers exactly the header
    assert sorted(L.SIGNATURES) == names


def header_prototypes(headers=("upr.h", "upr_train.h")):
    """name -> list of argument declarations, for every prototype in the headers."""
    protos = {}
    for h in headers:
        src = open(os.path.join(REPO, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
        for name, args in re.findall(r"\b(upr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
            args = " ".join(args.split())
            protos[name] = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
    return protos


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)


def test_signatures_match_header_arguments():
    """Arity and argument classes of the ctypes table against the C prototypes:
    a pointer exactly where the header has `*`, c_float exactly where it has
    `float`, and no c_int for a size_t / uint64_t."""
    protos = header_prototypes()
    assert sorted(protos) == header_functions()
    bad = []
    for name, decls in protos.items():
        args = L.SIGNATURES[name][1]
        if len(args) != len(decls):
            bad.append(f"{name}: {len(args)} argtypes, header has {len(decls)} arguments")
            continue
        for k, (t, d) in enumerate(zip(args, decls)):
            base = d.replace("const ", "").split()[0]
            if _is_pointer(t) != ("*" in d):
                bad.append(f"{name} arg {k} ({d}): pointer class differs ({t.__name__})")
            elif (t is ctypes.c_float) != ("*" not in d and base == "float"):
                bad.append(f"{name} arg {k} ({d}): float class differs ({t.__name__})")
            elif "*" not in d and base in ("size_t", "uint64_t") and t is ctypes.c_int:
                bad.append(f"{name} arg {k} ({d}): c_int for a 64-bit argument")
    assert not bad, "\n".join(bad)


# kernels that once had C linkage by accident (defined inside an extern "C" block)
FORMER_C_KERNELS = ("cast_act_f16_kernel", "cast_act_f32_kernel", "cast_f16_kernel", "chan_fin_bn_kernel",
                    "zero_view_kernel", "add16_kernel", "mse16_kernel")


def exported_symbols(path):
    """Names of the defined symbols in an ELF64 little-endian shared object's .dynsym."""
    import struct
    blob = open(path, "rb").read()
    assert blob[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for _, typ, _, _, off, size, link, _, _, entsize in secs:
        if typ != 11:  # SHT_DYNSYM
            continue
        stroff = secs[link][4]
        for o in range(off, off + size, entsize):
            st_name, _, _, shndx = struct.unpack_from("<IBBH", blob, o)
            if shndx:  # defined here
                names.append(blob[stroff + st_name:blob.index(b"\0", stroff + st_name)].decode())
    return names


def test_no_kernel_has_c_linkage():
    cdll = ctypes.CDLL(L.LIB_PATH)
    for k in FORMER_C_KERNELS:
        for sym in (k, "__device_stub__" + k):
            assert not hasattr(cdll, sym), f"{sym} is exported unmangled"
    # the invariant itself: kernel handles and host stubs are exported C++-mangled only (a mangled
    # name goes on with its parameter types, so a name that ends in _kernel has C linkage)
    syms = exported_symbols(L.LIB_PATH)
    assert sum(n.startswith("upr_") for n in syms) >= len(L.SIGNATURES)  # the reader sees the exports
    assert sum(n.startswith("_Z") and "_kernel" in n for n in syms) > 50  # ... and the kernels
    assert [n for n in syms if n.endswith("_kernel")] == []


def test_status_strings():
    assert L.status_string(0) == "ok"
    assert "shape" in L.status_string(L.UPR_ERR_SHAPE)
    assert "workspace" in L.status_string(L.UPR_ERR_WORKSPACE)


def test_lab_tables_match_oracle():
    a = cv_u8.lab_tables()
    b = runtime.lab_tables()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_null_args_rejected_without_device():
    lib = L.lib()
    assert lib.upr_model_workspace(None, 1, 64, 64) == 0
    assert lib.upr_model_forward(None, None, 1, 64, 64, None, None, None, None, 0, None) == L.UPR_ERR_ARG
    assert lib.upr_quantize_u8(None, None, 10, 0, None) == L.UPR_ERR_ARG
    assert lib.upr_clahe_u8(None, None, None, 1, 8, 8, 2.0, 8, 8, None) == L.UPR_ERR_ARG
    assert lib.upr_conv2d_nhwc(None, 1, 8, 8, 32, None, None, 32, 3, 3, 1, 1, 1, None, 0, None, 0, None) \
        == L.UPR_ERR_ARG
    out = ctypes.c_void_p()
    assert lib.upr_model_create(None, 0, 0, 0, 7, 0, ctypes.byref(out)) == L.UPR_ERR_ARG
    # flags: at most one of IENET_ONLY (1) / HEAD_ONLY (2), no unknown bits -- refused
    # before the (empty) state_dict is even looked at, so before any device call
    for bad in (3, 4, 8, 1 << 20, -1):
        assert lib.upr_model_create(None, 0, 0, 0, 0, bad, ctypes.byref(out)) == L.UPR_ERR_ARG, bad
        assert not out.value
    # training entries (include/upr_train.h) validate before touching the device
    assert lib.upr_t_conv_mfma(None, 1, 8, 8, 32, 32, 0, None, None, 32, 3, 3, 1, 1, 1, None, 0, 0, None, 32, 0, 0,
                               None) == L.UPR_ERR_ARG
    assert lib.upr_t_conv_wgrad(None, 1, 8, 8, 31, 31, 0, None, 8, 8, 32, 32, 0, 3, 3, 1, 1, 1, None,
                                None) == L.UPR_ERR_ARG
    assert lib.upr_t_adam(None, None, None, None, 10, None, 1.0, 1e-4, 0.9, 0.999, 1e-8, 0.0, 1, None,
                          None) == L.UPR_ERR_ARG
    assert lib.upr_t_loss_workspace(2, 64, 64) > 0
    assert lib.upr_t_loss_workspace(2, 8, 8) == 0
    assert lib.upr_t_pointwise(None, None, None, 4, 0, None, None, 0.0, 0, None) == L.UPR_ERR_ARG
