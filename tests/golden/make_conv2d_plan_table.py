"""Produces tests/golden/conv2d_plan_table.json: what ``sec_conv2d_fwd_plan_name`` of a DEFAULT build answers over a grid of
layers, map sizes, dtypes and call forms, under each setting of the two process-wide switches.  The query is host-only (no GPU):

    python tests/golden/make_conv2d_plan_table.py [path to libsecond_hip.so]

The switches are read once per process, so every setting is queried in a child process of its own (``--query``).  The table pins
the dispatch of the dense conv2d forward: tests/test_conv2d_plan_table.py asserts exact equality, so a change of the dispatch code
that moves any answer has to be made on purpose (re-record and say why)."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv2d_plan_table.json")

# (ksize, stride, pad, cin, cout): the layers of the configured RPNs, one shape on each side of every channel condition, and a
# 5x5 / p0 layer whose output is empty on the 2 x 2 map
LAYERS = ([[3, 1, 1, ci, co] for ci, co in ([128, 128], [128, 256], [64, 128], [64, 64], [256, 256], [256, 128], [192, 128], [128, 192])]
          + [[3, 2, 1, ci, co] for ci, co in ([64, 64], [64, 128], [128, 128])]
          + [[4, 4, 0, 64, 128], [2, 2, 0, 128, 128]]
          + [[1, 1, 0, ci, co] for ci, co in ([128, 128], [128, 64], [256, 128], [384, 128], [64, 64])]
          + [[5, 1, 2, 320, 64], [5, 1, 0, 64, 64]])
# (batch, h, w): small and ragged maps, the configured ones, and a point on each side of every size threshold of the decision:
#   1 x 188 x 256 | 1 x 192 x 256   376 | 384 workgroups of the generic kernel's 128-wide form (cout 128)
#   16 | 17 x 128 x 128             1024 | 1088 workgroups: several rounds of the 64 -> 64 3x3 / s1 patch form
#   4 x 100 x 100 (cout 128 | 256)  700 | 1400: ... of the 256-channel one;  400 | (4 x 248 x 248) 1984: ... of the 2x2 / s2 deblock
#   4 x 200 x 200 | 4 x 400 x 400   364 | 1300: ... of the rows form;  4 x 800 x 800: 5000 > 2560 workgroups of the 64 -> 64 3x3 / s2 form
#   1672 x 1672 | 1673 x 1672, 2048 x 2047 | 2048 x 2048, 2896 x 2896 | 2896 x 2897, 4096 x 4095 | 4096 x 4096
#                                   a frame of 384 / 256 / 128 / 64 channels below | past 2^31 bytes (the 128-channel pair: the x3 planes too)
#   16384 x 16383 | 16384 x 16384   the gather form's two map planes, 23170 x 23170 | 23171 x 23171 the rows form's map
MAPS = [[1, 2, 2], [1, 16, 16], [1, 24, 20], [4, 50, 50], [4, 100, 100], [4, 200, 200], [8, 200, 176], [8, 124, 124], [4, 248, 248],
        [4, 400, 400], [4, 800, 800], [1, 188, 256], [1, 192, 256], [16, 128, 128], [17, 128, 128],
        [1, 1672, 1672], [1, 1673, 1672], [1, 2048, 2047], [1, 2048, 2048], [1, 2896, 2896], [1, 2896, 2897], [1, 4096, 4095], [1, 4096, 4096],
        [1, 16384, 16383], [1, 16384, 16384], [1, 23170, 23170], [1, 23171, 23171]]
DTYPES = [0, 1, 2]                      # SEC_F32 (every answer ""), SEC_F16, SEC_BF16 (include/second_hip.h)
FORMS = [0, 1, 2, 3, 4, 5, 6, 7]        # SEC_CONV2D_FORM_*: plain, into, rows, tiles / lazy, tail, x3, x3 tiles, gather
ENVS = [{}, {"SEC_CONV2D_PATCH": "0"}, {"SEC_CONV2D_MFMA": "32"}]
SWITCHES = ("SEC_CONV2D_PATCH", "SEC_CONV2D_MFMA")


def grid():
    """(batch, h, w, cin, cout, ksize, stride, pad, dtype, call_form) in the order of one setting's slice of the table."""
    for (ks, st, pad, cin, cout), (b, h, w), dt, form in itertools.product(LAYERS, MAPS, DTYPES, FORMS):
        yield b, h, w, cin, cout, ks, st, pad, dt, form


def query(lib_path):
    """This process's answers over the grid."""
    lib = ctypes.CDLL(lib_path)
    lib.sec_conv2d_fwd_plan_name.argtypes = [ctypes.c_int] * 10
    lib.sec_conv2d_fwd_plan_name.restype = ctypes.c_char_p
    return [lib.sec_conv2d_fwd_plan_name(*q).decode() for q in grid()]


def record(lib_path):
    """One list of names per setting of ENVS, each from a fresh child process (an ordinary subprocess)."""
    out = []
    for env in ENVS:
        child_env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        child_env.update(env)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--query", lib_path], env=child_env, stdout=subprocess.PIPE, check=True)
        out.append(json.loads(r.stdout))
    return out


def encode(per_env):
    """-> (sorted unique names, one list of indices into them per setting)"""
    names = sorted({n for names in per_env for n in names})
    index = {n: i for i, n in enumerate(names)}
    return names, [[index[n] for n in names_] for names_ in per_env]


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--query":
        json.dump(query(sys.argv[2]), sys.stdout)
        return
    lib_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "second.pytorch_amd", "lib", "libsecond_hip.so")
    names, plans = encode(record(lib_path))
    table = {"layers": LAYERS, "maps": MAPS, "dtype": DTYPES, "call_form": FORMS, "env": ENVS,
             "order": "env; then layer (ksize, stride, pad, cin, cout), map (batch, h, w), dtype, call_form (last fastest)",
             "names": names, "plans": [" ".join(map(str, p)) for p in plans]}
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(OUT, sum(len(p) for p in plans), "entries,", len(names), "names")


if __name__ == "__main__":
    main()
