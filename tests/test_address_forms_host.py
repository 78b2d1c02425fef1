"""The host side of the address forms of the aggregation kernels (32-bit buffer descriptor + 24-bit multiply | 32-bit global
offset | 64-bit addresses): the two rules of stag_amd/csrc/entry_args.hpp at every boundary, from a stand-alone program
(tests/host/address_forms_main.cpp, built here); the shapes of tests/test_gpu_address_forms.py on the side of each rule that
test means to run; and the refusal of a row stride of 2^32 bytes or more by the entry points of agg_common (api.hip), which
took it and truncated it.  No device is needed: nothing is dereferenced."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import test_entry_refusals_host as R
import test_gpu_address_forms as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENOSYS = -38


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The stand-alone program, compiled with the host's undefined-behaviour sanitizer (shifts, casts and overflows are
    what these rules are made of)."""
    exe = str(tmp_path_factory.mktemp("address_forms") / "address_forms")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-x", "hip", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "address_forms_main.cpp"),
                    "-o", exe], check=True)
    return exe


def _ask(program, *args):
    out = subprocess.run([program, *map(str, args)], check=True, capture_output=True, text=True).stdout.split()
    return [int(v) for v in out]


def test_both_rules_at_every_boundary(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and "0 missed" in r.stdout and not r.stderr, r.stdout + r.stderr


@pytest.mark.parametrize("form", list(G.FORMS))
def test_the_gpu_test_s_tables_fall_on_the_intended_side(program, form):
    """Every table of test_gpu_address_forms.py, through the rule of the entry points that gather it: wide where the form is
    meant to be wide, narrow (and of the intended extent) at the top of the narrow form, and the compact twin always narrow."""
    f = G.FORMS[form]
    m, E = len(f["sources"]), G.N_EDGES
    for D in f["widths"]:
        ldx = f["stride_bytes"] // 4
        rc, wide, x_bytes, _ = _ask(program, "agg", f["n_src"], E, ldx, D)
        assert rc == 0 and (wide & 2) == 0 and bool(wide & 1) == f["wide"], (form, D, wide)
        assert (x_bytes == 0) == f["wide"]
        rc, x_bytes = _ask(program, "rows", f["n_src"], ldx, D, 4)
        assert rc == 0 and (x_bytes == 0) == f["wide"], (form, D, x_bytes)
        if form == "d":
            assert x_bytes >= (1 << 31), "the top of the narrow form: offsets that use all 32 bits"
        assert _ask(program, "agg", m, E, D, D)[1] == 0 and _ask(program, "rows", m, D, D, 4)[1] > 0      # the compact twin
    ldx = f["stride_bytes"] // 2
    rc, x_bytes = _ask(program, "rows", f["n_src"], ldx, G.HALF_D, 2)
    assert rc == 0 and (x_bytes == 0) == f["wide"], (form, "half", x_bytes)
    assert _ask(program, "rows", m, G.HALF_D, G.HALF_D, 2)[1] > 0
    # what the form is about, and nothing else
    last = (f["n_src"] - 1) * f["stride_bytes"]
    assert max(f["sources"]) == f["n_src"] - 1 and min(f["sources"]) == 0
    assert (f["n_src"] >= 1 << 24) == (form == "a") and (f["stride_bytes"] >= 1 << 24) == (form == "b")
    assert (last >= 1 << 32) == (form == "c") and ((1 << 31) <= last < (1 << 32)) == (form == "d")
    for bound in f["straddles"]:        # byte offsets with a gathered row on either side
        offs = [s * f["stride_bytes"] for s in f["sources"]]
        assert any(o < bound for o in offs) and any(o >= bound for o in offs), (form, bound)
        assert bound - f["stride_bytes"] in offs and bound in offs


def test_the_per_edge_graph_falls_on_the_intended_side(program):
    E, n = G.PE_EDGES, G.PE_N_SRC
    assert E >= (1 << 24) and E * 4 * 4 < (1 << 32) <= E * 64 * 4
    for D in (4, 64):
        rc, wide, x_bytes, idx_bytes = _ask(program, "agg", n, E, D, D)
        assert rc == 0 and wide == 2 and x_bytes == n * D * 4 and idx_bytes == E * 4      # the per-edge rows only
        assert _ask(program, "rows", n, D, D, 4) == [0, n * D * 4]
    assert _ask(program, "agg", n, (1 << 24) - 1, 4, 4)[1] == 0


# ---- the refusal ------------------------------------------------------------------------------------------------------
STRIDED = [("stag_agg_fwd", "ldx"), ("stag_agg_fwd_mc", "ldx"), ("stag_agg_bwd", "ldx"), ("stag_agg_bwd_edge", "ldg"),
           ("stag_agg_bwd_dp", "ldg")]


@pytest.mark.parametrize("name,ld", STRIDED)
def test_a_row_stride_of_2_32_bytes_is_refused(name, ld):
    """The base call of test_entry_refusals_host.py with the gathered table's stride at 2^30 floats: STAG_ENOSYS before any
    device work (the kernels take the stride as 32 bits of bytes; the call used to go through and gather row 0 for every
    source).  One float less is a stride the 64-bit form takes, so it must not be refused: replayed where no device is
    present, as a call that passes every check launches on dummy pointers."""
    from stag_amd import _lib
    assert ld in R.ENTRIES[name][0]
    call = R.base_call(name)
    call[ld] = 1 << 30
    assert R.run(_lib.lib(), _lib, name, call) == ENOSYS
    call[ld] = 1 << 40
    assert R.run(_lib.lib(), _lib, name, call) == ENOSYS
    if not torch.cuda.is_available():
        call[ld] = (1 << 30) - 1
        assert R.run(_lib.lib(), _lib, name, call) not in (R.EINVAL, R.ENOSYS, R.ENOMEM)


def test_a_refusal_recorded_before_the_stride_keeps_its_code():
    """The new refusal stands behind the argument checks it follows in agg_common: a bad csr or spec is still STAG_EINVAL."""
    from stag_amd import _lib
    for name, ld in STRIDED:
        for arg, fields in (("csr" if "csr" in R.ENTRIES[name][0] else "csr_t", dict(n_dst=-1)), ("spec", dict(kind=9))):
            call = R.base_call(name)
            call[ld] = 1 << 30
            call[arg].update(fields)
            assert R.run(_lib.lib(), _lib, name, call) == R.EINVAL, (name, arg)


def test_ops_packs_a_single_row_whose_view_carries_such_a_stride():
    """torch calls one row contiguous whatever its stride, so contiguous() alone would hand the stride down."""
    from stag_amd import ops
    flat = torch.zeros(16)
    x = flat.as_strided((1, 8), (1 << 30, 1))
    assert x.is_contiguous() and x.stride(0) == 1 << 30
    packed = ops._f32c(x)
    assert packed.stride(0) == 8 and torch.equal(packed, x)
    y = torch.arange(32.0).reshape(4, 8)
    assert ops._f32c(y) is y
