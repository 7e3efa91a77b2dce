"""The ABI layout self-check, for every descriptor struct at once (no GPU): the header, the ctypes mirrors of detr_tf/_hip.py, what
detr_hip_struct_layout reports and the frozen layouts of tests/golden/abi_layouts.json agree; unknown ids are rejected; a drifted mirror
is caught by the load-time check.  What is particular to one descriptor (array sizes, field groups, #defines) is in its feature's file."""
import ctypes
import functools
import json

import pytest

import abi_header as H

_lib = H.hip_lib
IDS = sorted(H.C_NAMES)                                                        # the test's own list: the registry is held to it
each_id = pytest.mark.parametrize("which", IDS)


@functools.lru_cache(maxsize=None)
def _gcc_layouts():
    """One compile for all structs: the header's layout of every mirror's field names."""
    return H.header_layouts({H.C_NAMES[w]: [f for f, _ in S._fields_] for w, S in sorted(_lib()[0].LAYOUT_STRUCTS.items())})


def test_registry_is_complete():
    _hip, _ = _lib()
    assert sorted(_hip.LAYOUT_STRUCTS) == IDS == list(range(10)) + [100, 200, 300, 400, 500, 600, 700, 800]
    assert {w: S.__name__ for w, S in _hip.LAYOUT_STRUCTS.items()} == {
        0: "ReduceDesc", 1: "GemmDesc", 2: "Conv3x3Desc", 3: "StemDesc", 4: "LayerNormDesc", 5: "AttnDesc", 6: "SetLossDesc", 7: "InputDesc",
        8: "PostprocessDesc", 9: "MapMatchDesc", 100: "DetectDesc", 200: "TileMergeDesc", 300: "OverlayDesc", 400: "TrackDesc",
        500: "TrackEmbedDesc", 600: "TrackMotionDesc", 700: "Conv3x3DDesc", 800: "CocoMatchDesc"}
    mirrors = {v for k, v in vars(_hip).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and k.endswith("Desc")}
    assert mirrors == set(_hip.LAYOUT_STRUCTS.values()) and len(mirrors) == 18                 # no mirror escapes the load-time check
    assert sorted(H.header_structs()) == sorted(H.C_NAMES.values())                            # nor does a struct of the header
    assert not [k for k in vars(_hip) if k.startswith("LAYOUT_STRUCTS") and k != "LAYOUT_STRUCTS"]


@each_id
def test_header_equals_the_mirror(which):
    """Independent of the library: sizeof / offsetof as gcc lays the header out, and the names, order and types of the C declaration
    (the parser copes with all 18 structs), are the mirror's."""
    _hip, _ = _lib()
    S = _hip.LAYOUT_STRUCTS[which]
    assert _gcc_layouts()[H.C_NAMES[which]] == _hip.struct_layout_mirror(S)
    assert H.header_structs()[H.C_NAMES[which]] == [(f, ctypes.c_void_p if issubclass(t, ctypes._Pointer) else t) for f, t in S._fields_]


@each_id
def test_library_layout_equals_the_mirror(which):
    _hip, lib = _lib()
    S = _hip.LAYOUT_STRUCTS[which]
    want = _hip.struct_layout_mirror(S)
    buf = (ctypes.c_int32 * 96)()
    n = lib.detr_hip_struct_layout(which, buf, 96)
    assert n == len(want) == 1 + len(S._fields_) <= 96 and list(buf[:n]) == want
    assert H.library_layout(lib, which) == want                                 # sized by the returned count
    short = (ctypes.c_int32 * 3)(-1, -1, -1)                                    # a short buffer: the same count, two values written
    assert lib.detr_hip_struct_layout(which, short, 2) == n and list(short) == want[:2] + [-1]


@pytest.mark.parametrize("which", [w + 1 for w in IDS if w + 1 not in IDS] + [99, -1])
def test_unknown_ids_are_rejected(which):
    _hip, lib = _lib()
    buf = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    assert lib.detr_hip_struct_layout(which, buf, 4) < 0 and list(buf) == [-1] * 4
    assert lib.detr_hip_last_error().decode() == f"struct_layout: unknown struct {which}"


@each_id
def test_a_drifted_mirror_is_caught_at_load(which):
    _hip, lib = _lib()
    S = _hip.LAYOUT_STRUCTS[which]
    _hip.check_struct_layouts(lib)                                              # the load-time check passes as it stands
    wide = {ctypes.c_int32: ctypes.c_int64, ctypes.c_uint32: ctypes.c_int64, ctypes.c_float: ctypes.c_double}
    for victim, _ in S._fields_:               # the first field whose widening (4 -> 8 bytes, or to 16) moves an offset or the size:
        class Drifted(ctypes.Structure):       # padding absorbs some, e.g. an int32_t in front of a pointer
            _fields_ = [(f, wide.get(ft, ctypes.c_int64 * 2) if f == victim else ft) for f, ft in S._fields_]
        if _hip.struct_layout_mirror(Drifted) != _hip.struct_layout_mirror(S):
            break
    try:
        _hip.LAYOUT_STRUCTS[which] = Drifted
        with pytest.raises(RuntimeError, match=rf"struct {which} \(Drifted\)"):
            _hip.check_struct_layouts(lib)
    finally:
        _hip.LAYOUT_STRUCTS[which] = S
    _hip.check_struct_layouts(lib)


def test_library_layouts_are_the_frozen_ones():
    """tests/golden/abi_layouts.json (scripts/record_abi_layouts.py) is the ABI: a value that moves is a break, a new id adds a line."""
    _, lib = _lib()
    golden = {int(k): v for k, v in json.load(open(H.GOLDEN)).items()}
    assert sorted(golden) == IDS
    for which in IDS:
        assert H.library_layout(lib, which) == golden[which], H.C_NAMES[which]
