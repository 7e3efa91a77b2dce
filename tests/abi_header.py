"""The descriptor structs of include/detr_hip.h as a test sees them: one parser of their C declarations, and one C program, compiled
with the header, that prints sizeof and every offsetof.  Shared by tests/test_abi_layout_cpu.py, the feature tests that look at one
struct's fields, and scripts/record_abi_layouts.py.  Neither half asks the library."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "detr_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_layouts.json")
# detr_hip_struct_layout's ids (ABI: they never change) -> the C name of the struct
C_NAMES = {0: "detr_reduce_desc", 1: "detr_gemm_desc", 2: "detr_conv3x3_desc", 3: "detr_stem_desc", 4: "detr_layernorm_desc",
           5: "detr_attn_desc", 6: "detr_setloss_desc", 7: "detr_input_desc", 8: "detr_postprocess_desc", 9: "detr_map_match_desc",
           100: "detr_detect_desc", 200: "detr_tile_merge_desc", 300: "detr_overlay_desc", 400: "detr_track_desc",
           500: "detr_track_embed_desc", 600: "detr_track_motion_desc", 700: "detr_conv3x3d_desc", 800: "detr_coco_match_desc"}
SCALARS = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
           "double": ctypes.c_double}


def hip_lib():
    """(detr_tf._hip, the loaded library), built first where it is missing."""
    from detr_tf import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip, _hip.load()


@functools.lru_cache(maxsize=None)
def header_structs():
    """{C name: [(field, ctypes type)]} of every `typedef struct ... detr_*_desc`, in declaration order.  A pointer of any type is
    c_void_p; an array is scalar * length, with the DETR_* macros of the header resolved."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    macros = {name: int(value) for name, value in re.findall(r"^#define (DETR_\w+) (\d+)[ \t]*$", text, flags=re.M)}
    structs = {}
    for body, name in re.findall(r"typedef struct(?: \w+)? \{([^}]*)\} (detr_\w+_desc);", text):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, items = re.fullmatch(r"(?:const\s+)?(?:struct\s+)?(\w+)\s+(.*)", decl, flags=re.S).groups()
            for item in (i.strip() for i in items.split(",")):
                star, field, length = re.fullmatch(r"(\*?)\s*(\w+)(?:\[([^\]]+)\])?", item).groups()
                ctype = ctypes.c_void_p if star else SCALARS[base]
                if length is not None:
                    length = re.sub(r"DETR_\w+", lambda m: str(macros[m.group(0)]), length)
                    assert re.fullmatch(r"[\d\s*]+", length), (name, item)
                    ctype = ctype * eval(length)
                fields.append((field, ctype))
        structs[name] = fields
    return structs


def header_layouts(names_by_struct):
    """{C name: [sizeof, offsetof(field 0), ...]} as gcc lays the header's structs out, for the field names given per struct: one
    generated C program that is compiled and run."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "detr_hip.h"', "int main(void) {"]
    for cname, names in names_by_struct.items():
        lines.append(f'  printf("%zu", sizeof({cname}));')
        lines += [f'  printf(" %zu", offsetof({cname}, {n}));' for n in names]
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}", ""]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), src, "-o", exe])
        rows = subprocess.check_output([exe]).decode().splitlines()
    assert len(rows) == len(names_by_struct)
    return {cname: [int(v) for v in row.split()] for cname, row in zip(names_by_struct, rows)}


def library_layout(lib, which):
    """What detr_hip_struct_layout reports for id `which` (None: unknown id), sized by the count it returns."""
    n = lib.detr_hip_struct_layout(which, None, 0)
    if n < 0:
        return None
    buf = (ctypes.c_int32 * n)()
    assert lib.detr_hip_struct_layout(which, buf, n) == n
    return list(buf)
