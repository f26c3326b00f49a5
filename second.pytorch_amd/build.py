"""Build libsecond_hip.so (all HIP kernels + the C ABI) for gfx950 with hipcc, in-tree.

    python second.pytorch_amd/build.py [--force]

hipcc cross-compiles without a GPU.  The library lands in second.pytorch_amd/lib/ (git-ignored, but it
travels to the GPU box with the gpurun snapshot).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = [os.path.join(HERE, "csrc", f) for f in
       ("common.hip", "voxelize.hip", "rulebook.hip", "indice_conv.hip", "scatter.hip", "nms.hip", "dense.hip", "dense_f32.hip", "pillars.hip", "predict.hip", "train.hip", "dense_train.hip", "augment.hip", "anchor_mask.hip", "kitti_eval.hip", "kitti_annos.hip", "train_metrics.hip")]
HDR = [os.path.join(HERE, "csrc", "common.hpp"), os.path.join(HERE, "csrc", "dense_patch.hpp"), os.path.join(HERE, "csrc", "rotated_clip.hpp"), os.path.join(HERE, "..", "include", "second_hip.h")]
OUT = os.path.join(HERE, "lib", "libsecond_hip.so")
# No packed fp32 VALU: `-Xclang -target-feature -Xclang -packed-fp32-ops` makes the backend split every <2 x float> operation, so no
# v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 is emitted (the vectorisers stay on: they also merge loads / stores, worth 9-15 % on the
# 64-channel sparse-conv kernels).  On gfx950 (ROCm 7.2) those instructions were measured to return WRONG results in lanes 48..63 of a
# wave -- a product term missing -- while another wave of the CU runs the dense v_mfma_f32_32x32x16_bf16 loop of the RPN conv kernel
# (tools/nms_stress.py: the rotated-NMS clipper's corner arithmetic differed in ~1 % of its evaluations beside k_conv2d_halo_reg;
# 0 of 400 runs without packed fp32).  The cause was never isolated (every instruction-level probe came back clean), so the rule is
# a blanket one: NO kernel of this library uses packed fp32 -- the one exemption (k_conv_rows_buf, rounds 2-4) was dropped in round 5
# when an A/B showed it bought nothing any more (profiles/r05_b_packed_fp32_exemption_ab.txt); tests/test_gpu_stress.py replays the
# bench configuration 600 steps and the NMS 500 times beside the RPN conv.  The host pass of hipcc prints "not a recognized feature"
# for the flag (filtered below).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
         "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]


def build(force=False, verbose=True, tag=None, extra_flags=None):
    """``tag`` / ``extra_flags`` (or SEC_BUILD_TAG / SEC_EXTRA_HIPCC_FLAGS): a profiling build next to the shipped library,
    e.g. tag "tl" + -DSEC_CONV_TIMELINE -> lib/libsecond_hip_tl.so, loaded with SEC_HIP_LIB=<that path>."""
    tag = tag or os.environ.get("SEC_BUILD_TAG", "")
    out_path = OUT.replace(".so", f"_{tag}.so") if tag else OUT
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    exp_dir = os.path.join(HERE, "..", "tools", "kernel_experiments")      # A/B kernels of -DSEC_CONV_EXPERIMENTS builds: outside the product tree
    hdrs = HDR + ([os.path.join(exp_dir, f) for f in os.listdir(exp_dir)] if os.path.isdir(exp_dir) else [])
    if not force and os.path.exists(out_path):
        newest = max(os.path.getmtime(p) for p in SRC + hdrs)
        if os.path.getmtime(out_path) >= newest:
            return out_path
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = list(extra_flags) if extra_flags is not None else os.environ.get("SEC_EXTRA_HIPCC_FLAGS", "").split()   # e.g. -DSEC_CONV_ABLATIONS
    # one translation unit per source, compiled concurrently (indice_conv.hip / dense.hip dominate), then one link
    from concurrent.futures import ThreadPoolExecutor
    objdir = os.path.join(HERE, "lib", "obj_" + tag if tag else "obj")
    os.makedirs(objdir, exist_ok=True)
    cflags = [f for f in FLAGS if f != "-shared"]

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        cmd = [hipcc, *cflags, *extra, "-c", "-o", obj, src]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        err = "\n".join(l for l in r.stderr.splitlines() if "is not a recognized feature for this target" not in l)
        if err.strip():
            print(err, file=sys.stderr, flush=True)
        if r.returncode:
            raise subprocess.CalledProcessError(r.returncode, cmd)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(SRC), os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, SRC))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fvisibility=hidden", "-o", out_path, *objs]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out_path


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
