"""Produces tests/golden/conv_plan_table.json: what ``sec_indice_conv_fwd_plan`` of a DEFAULT build answers over a grid of
shapes, row counts, dtypes and variant numbers.  The query is host-only (no GPU):

    python tests/golden/make_conv_plan_table.py [path to libsecond_hip.so]

The table pins the dispatch of the sparse-conv forward: tests/test_conv_plan_table.py asserts exact equality, so a change of
the dispatch code that moves any answer has to be made on purpose (re-record and say why)."""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv_plan_table.json")

# the shapes the 16-bit MFMA path serves, the first layer (4 -> 16) and two shapes without a specialised kernel
SHAPES = [[16, 16], [16, 32], [32, 32], [32, 64], [64, 64], [64, 128], [128, 128], [16, 64], [64, 32], [32, 16], [128, 64],
          [4, 16], [3, 16], [5, 7]]
KVOLS = [27, 3]
ROWS = [1, 6000, 8191, 8192, 39999, 40000, 60000]
DTYPES = [0, 1, 2]                      # SEC_F32, SEC_BF16, SEC_F16 (include/second_hip.h)
OUT_F32 = [0, 1]                        # out_dtype = dtype | SEC_F32
PACKED = [0, 1]
VARIANTS = [-1, 0, 1, 8, 9, 22, 29, 30, 31, 32, 41, 46, 50, 80, 81, 82, 83]


def grid():
    """(variant, cin, cout, kvol, rows, dtype, out_dtype, has_packed) in the order of the table's `plans` list."""
    for v, (cin, cout), kvol, rows, dt, of32, packed in itertools.product(VARIANTS, SHAPES, KVOLS, ROWS, DTYPES, OUT_F32, PACKED):
        yield v, cin, cout, kvol, rows, dt, (0 if of32 else dt), packed


def record(lib_path):
    lib = ctypes.CDLL(lib_path)
    lib.sec_indice_conv_fwd_plan.argtypes = [ctypes.c_int] * 7
    lib.sec_indice_conv_set_variant.argtypes = [ctypes.c_int]
    plans, cur = [], None
    try:
        for v, *q in grid():
            if v != cur:
                lib.sec_indice_conv_set_variant(v)
                cur = v
            plans.append(int(lib.sec_indice_conv_fwd_plan(*q)))
    finally:
        lib.sec_indice_conv_set_variant(-1)
    return plans


def main():
    lib_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "second.pytorch_amd", "lib", "libsecond_hip.so")
    table = {"shapes": SHAPES, "kvol": KVOLS, "rows": ROWS, "dtype": DTYPES, "out_f32": OUT_F32, "has_packed": PACKED,
             "variants": VARIANTS, "order": "variant, shape, kvol, rows, dtype, out_f32, has_packed (last fastest)",
             "plans": "".join("%02d" % p for p in record(lib_path))}
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(OUT, len(table["plans"]) // 2, "entries")


if __name__ == "__main__":
    main()
