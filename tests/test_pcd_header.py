"""fdm_pcd_parse_header / fdm_pcd_write_header (fastdem_amd/csrc/fdm_pcd_host.hpp behind the C ABI) against the restatement
of nanoPCL's parseHeader and savePCD (tests/pcd_restate.py): every value of the header equal, an error where the
restatement raises.  Host code only: no device is touched."""
import ctypes as C

import numpy as np
import pytest

import pcd_cases as PC
import pcd_restate as PR


@pytest.fixture(scope="module")
def pcd():
    from fastdem_amd import pcd
    return pcd


def engine_parse(pcd, data):
    from fastdem_amd import EngineError
    try:
        return PC.engine_tuple(pcd.parse_header(data))
    except EngineError:
        return None


@pytest.mark.parametrize("name", sorted(PC.HEADERS))
def test_header_cases(pcd, name):
    data = PC.HEADERS[name]
    want = PC.restated(data)
    assert engine_parse(pcd, data) == want
    more = data + b"1 2 3 4 5 6 7 8 9 10 11\nWIDTH 77\n"
    assert engine_parse(pcd, more) == PC.restated(more)
    if b"\nDATA" in data and data.endswith(b"\n") and want is not None:
        assert PC.restated(more) == want                                 # what follows the DATA line is not looked at


def test_the_cases_cover_errors_and_parses():
    errors = sorted(k for k, v in PC.HEADERS.items() if PC.restated(v) is None)
    assert errors == ["binary_compressed", "empty", "fields_65", "height_without_number", "no_fields", "size_not_a_number",
                      "viewpoint_not_a_number", "width_not_a_number", "width_without_number"]
    t = PC.restated(PC.HEADERS["crlf"])
    assert t[0][4] == ("rgb", "U", 4, 1, 16) and t[1:4] == (12, 3, 20) and t[4] == (1, 2, 3, 0.5, 0.5, -0.5, 0.5)
    assert PC.restated(PC.HEADERS["short_lists"])[0] == [("x", "F", 8, 1, 0), ("y", "F", 8, 1, 8), ("z", "F", 4, 2, 16),
                                                         ("intensity", "F", 4, 1, 24)]
    assert PC.restated(PC.HEADERS["pcl_xyzrgbnormal"])[3] == 48
    assert PC.restated(PC.HEADERS["count4_padding"])[0][4] == ("intensity", "F", 4, 1, 16)      # behind a `_` of COUNT 4
    assert PC.restated(PC.HEADERS["alias_intensity_first"])[7] == (1, 3, 5, 4, -1, -1, -1, -1)
    assert PC.restated(PC.HEADERS["nx_ny_without_nz"])[7][5:] == (3, 4, -1)


@pytest.mark.parametrize("name", ["valid", "crlf", "pcl_xyzrgbnormal", "viewpoint_eight_numbers"])
def test_truncated_at_every_byte(pcd, name):
    """The buffer handed over ends exactly at the cut (a NumPy copy of that size): an error or a parse, the
    restatement's.  (That no byte behind it is read is what tests/test_pcd_host_sanitized.py checks.)"""
    data = PC.HEADERS[name]
    seen = set()
    for cut in range(len(data) + 1):
        want = PC.restated(data[:cut])
        assert engine_parse(pcd, data[:cut]) == want, cut
        seen.add(want is None)
    assert seen == {True, False}


def test_null_arguments(pcd):
    from fastdem_amd import capi
    lib = capi.load()
    h = capi.FdmPcdHeader()
    assert lib.fdm_pcd_parse_header(None, 0, C.byref(h)) == capi.FDM_ERR_INVALID        # an empty file has no FIELDS
    assert lib.fdm_pcd_parse_header(None, 5, C.byref(h)) == capi.FDM_ERR_INVALID
    assert lib.fdm_pcd_parse_header(b"FIELDS x\n", 9, None) == capi.FDM_ERR_INVALID
    assert b"FIELDS" in lib.fdm_last_error() or b"null" in lib.fdm_last_error()


CHANNEL_SETS = [(False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True)]


@pytest.mark.parametrize("hi,hc,hn", CHANNEL_SETS)
@pytest.mark.parametrize("fmt", [PR.ASCII, PR.BINARY])
def test_write_header(pcd, hi, hc, hn, fmt):
    for n, vp in ((0, None), (3, (0, 0, 0, 1, 0, 0, 0)), (2 ** 31 - 1, (1.5, -2.25, 1e-7, 0.70710678118654757, 0, 0.70710678118654746, 0)),
                  (12345678, (123456789.0, 1e20, -1e-5, 0.1234565, 0.5, -0.5, 1 / 3))):
        want = PR.save_header(n, hi, hc, hn, vp, fmt)
        assert pcd.write_header(n, hi, hc, hn, vp, fmt) == want
        back = pcd.parse_header(want)                                      # and the parser reads it back
        assert (back.width, back.height, back.format, back.data_offset) == (n, 1, fmt, len(want))
        assert back.point_size == 12 + 4 * hi + 4 * hc + 12 * hn


def test_write_header_into_a_small_buffer(pcd):
    from fastdem_amd import capi
    lib = capi.load()
    want = PR.save_header(7, True, False, False, None, PR.BINARY)
    buf = C.create_string_buffer(b"\xAA" * len(want), len(want))
    need = C.c_uint64(0)
    assert lib.fdm_pcd_write_header(7, 1, 0, 0, None, 1, buf, len(want) - 1, C.byref(need)) == capi.FDM_SKIP_BUFFER_TOO_SMALL
    assert need.value == len(want) and buf.raw == b"\xAA" * len(want)
    assert lib.fdm_pcd_write_header(7, 1, 0, 0, None, 1, buf, len(want), C.byref(need)) == 0 and buf.raw == want
    assert lib.fdm_pcd_write_header(7, 1, 0, 0, None, 2, buf, len(want), C.byref(need)) == capi.FDM_ERR_INVALID


def test_header_struct_layout():
    from fastdem_amd import capi
    assert C.sizeof(capi.FdmPcdField) == 80 and C.sizeof(capi.FdmPcdHeader) == 64 * 80 + 16 + 56 + 36 + 4 + 8
    assert capi.FdmPcdHeader.data_offset.offset % 8 == 0 and capi.FdmPcdHeader.viewpoint.offset == 64 * 80 + 16
