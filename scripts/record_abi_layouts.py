"""Record the descriptor layouts of the library that is built in this tree: for every id of tests/abi_header.py: C_NAMES, the values
detr_hip_struct_layout reports (sizeof, then every offsetof in declaration order).  Writes tests/golden/abi_layouts.json
(tests/test_abi_layout_cpu.py compares the library with it).

An id the library does not know yet is recorded from the header instead: a C program compiled with include/detr_hip.h prints the same
values for the fields the header declares.  Where each id of the committed file came from:
    0..9, 100, 200, 300, 400, 500, 600   the library built at the commit BEFORE detr_hip_struct_layout became a table (a switch with
                                         one statement per field), so the file proves that the rewrite moved no value;
    700, 800                             the header, through gcc: that library did not report them.

Host code only: runs without a GPU.  Run it BEFORE a change that is meant to keep the ABI and commit the file unchanged with that change;
a descriptor that is new, or a field appended to one, adds or lengthens a line and changes no other.

    python scripts/record_abi_layouts.py [--lib detr-tensorflow_amd/lib/libdetr_hip.so] [--out tests/golden/abi_layouts.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import abi_header as H
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "detr-tensorflow_amd", "lib", "libdetr_hip.so"))
    ap.add_argument("--out", default=H.GOLDEN)
    args = ap.parse_args()
    lib = ctypes.CDLL(args.lib)
    layouts = {which: H.library_layout(lib, which) for which in H.C_NAMES}
    missing = [which for which, values in layouts.items() if values is None]
    structs = H.header_structs()
    from_header = H.header_layouts({H.C_NAMES[w]: [f for f, _ in structs[H.C_NAMES[w]]] for w in missing}) if missing else {}
    for which in missing:
        layouts[which] = from_header[H.C_NAMES[which]]
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f'"{which}": {json.dumps(values)}' for which, values in layouts.items()) + "\n}\n")
    assert {int(k): v for k, v in json.load(open(args.out)).items()} == layouts
    print(f"{args.out}: {len(layouts)} structs, {len(missing)} of them from the header {missing}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
