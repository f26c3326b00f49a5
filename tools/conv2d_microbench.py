#!/usr/bin/env python3
"""Micro-benchmark of sec_conv2d_nhwc on the car.fhd RPN layer (3x3, 128->128, 8 x 200 x 176) vs MIOpen.
FP32=1 adds the fp32 rows: sec_conv2d_nhwc_f32 on every tile, sec_conv2d_nhwc_f32_tiles on LIVE_SHARE (default 0.33, the bench
clouds' 26-39 %) of the tiles -- lazy form and background-copying form -- and F.conv2d fp32 channels-last; fraction of the 157.3 TF
fp32 matrix peak beside each."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "second.pytorch_amd"))
import torch
from second_amd import ops
torch.manual_seed(0)
x = torch.randn(8, 128, 200, 176, device="cuda")
density = float(os.environ.get("DENSITY", "1.0"))   # fraction of non-zero pixels (the real RPN input is ~3 % dense)
if density < 1.0:
    x = x * (torch.rand(8, 1, 200, 176, device="cuda") < density)
x = x.bfloat16().contiguous(memory_format=torch.channels_last)
w = (torch.randn(128, 128, 3, 3, device="cuda") / 34).bfloat16()
b = torch.randn(128, device="cuda")
pk = ops.conv2d_pack_weight(w)
WARM, N = int(os.environ.get("WARM", "300")), int(os.environ.get("ITERS", "100"))
def bench(fn, n=N):
    for _ in range(WARM): fn()          # ~0.1 s of warm-up: the first launches of a process run at idle clocks
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n
ZSKIP = bool(int(os.environ.get("ZSKIP", "0")))   # flag the input as a scattered sparse tensor (all-zero tiles skipped)
t = bench(lambda: ops.conv2d_nhwc(x, pk, b, 128, 3, 1, 1, relu=True, sparse_input=ZSKIP))
flop = 2 * 8 * 200 * 176 * 128 * 128 * 9
print(f"density={density} zskip={int(ZSKIP)} hip: {t:.1f} us  {flop / t / 1e6:.0f} TFLOP/s")
if os.environ.get("WITH_MIOPEN"):
    wcl = w.contiguous(memory_format=torch.channels_last)
    t = bench(lambda: ops.bias_act_(torch.nn.functional.conv2d(x, wcl, None, 1, 1), b, True))
    print(f"miopen conv + fused bias/relu: {t:.1f} us  {flop / t / 1e6:.0f} TFLOP/s")
if os.environ.get("FP32"):
    PEAK = 157.3
    xf = x.float().contiguous(memory_format=torch.channels_last)
    wf = w.float()
    pkf = ops.conv2d_pack_weight_f32(wf)
    t = bench(lambda: ops.conv2d_nhwc_f32(xf, pkf, b, 128, relu=True, sparse_input=ZSKIP))
    print(f"fp32 hip, every tile: {t:.1f} us  {flop / t / 1e6:.1f} TFLOP/s  {flop / t / 1e6 / PEAK:.2f} of the fp32 matrix peak")
    share = float(os.environ.get("LIVE_SHARE", "0.33"))
    tiles = 25 * 11
    n_live = int(round(share * tiles))
    order = torch.stack([torch.randperm(tiles) for _ in range(8)]).to(torch.int16).cuda()
    counts = torch.full((8,), n_live, dtype=torch.int32, device="cuda")
    bg = ops.conv2d_nhwc_f32(torch.zeros_like(xf[:1]), pkf, b, 128, relu=True)
    lflop = flop * n_live / tiles
    t = bench(lambda: ops.conv2d_nhwc_f32_tiles(xf, pkf, b, 128, order, counts, relu=True))
    print(f"fp32 hip, {8 * n_live} live tiles of {8 * tiles}, lazy: {t:.1f} us  {lflop / t / 1e6:.1f} TFLOP/s on its tiles  {lflop / t / 1e6 / PEAK:.2f} of peak")
    t = bench(lambda: ops.conv2d_nhwc_f32_tiles(xf, pkf, b, 128, order, counts, background=bg, relu=True))
    print(f"fp32 hip, {8 * n_live} live tiles of {8 * tiles}, background copied: {t:.1f} us  {lflop / t / 1e6:.1f} TFLOP/s on its tiles")
    wfcl = wf.contiguous(memory_format=torch.channels_last)
    t = bench(lambda: ops.bias_act_(torch.nn.functional.conv2d(xf, wfcl, None, 1, 1), b, True))
    print(f"fp32 F.conv2d channels-last + fused bias/relu: {t:.1f} us  {flop / t / 1e6:.1f} TFLOP/s  {flop / t / 1e6 / PEAK:.2f} of peak")
if os.environ.get("AB_LOOPS"):
    # Both main loops of the 128-channel conv INTERLEAVED in one process (same clocks, same box state): the switch SEC_CONV2D_MFMA is
    # read once per loaded library, so a second copy of the library is loaded and latched on the 32x32x16 loop.  Post-ReLU inputs.
    import ctypes, shutil, tempfile
    from second_amd import runtime as rt
    xr = torch.relu(torch.randn(8, 128, 200, 176, device="cuda")).bfloat16().contiguous(memory_format=torch.channels_last)
    y = torch.empty_like(xr)
    tmp = tempfile.mkdtemp()
    lib32 = ctypes.CDLL(shutil.copy(rt.LIB_PATH, os.path.join(tmp, "libsecond_hip_mfma32.so")))
    lib32.sec_last_kernel_name.restype = ctypes.c_char_p
    P, I = ctypes.c_void_p, ctypes.c_int
    def run(l):
        rc = l.sec_conv2d_nhwc(P(xr.data_ptr()), I(8), I(200), I(176), I(128), P(pk.data_ptr()), P(b.data_ptr()), I(128), I(3), I(1), I(1), I(1),
                               P(y.data_ptr()), I(rt.dtype_code(xr.dtype)), P(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    assert "SEC_CONV2D_MFMA" not in os.environ
    run(rt.lib())                                     # latches the default loop
    os.environ["SEC_CONV2D_MFMA"] = "32"
    run(lib32)
    del os.environ["SEC_CONV2D_MFMA"]
    names = {"16x16x32": rt.lib().sec_last_kernel_name().decode(), "32x32x16": lib32.sec_last_kernel_name().decode()}
    print("loops:", names)
    assert ", 128, 8, 3, " in names["16x16x32"] and ", 128, 8, 2, " in names["32x32x16"]
    for rnd in range(int(os.environ.get("AB_ROUNDS", "4"))):
        t32 = bench(lambda: run(lib32))
        t16 = bench(lambda: run(rt.lib()))
        print(f"round {rnd}: 32x32x16 {t32:.2f} us  {flop / t32 / 1e6:.0f} TFLOP/s | 16x16x32 {t16:.2f} us  {flop / t16 / 1e6:.0f} TFLOP/s | ratio {t16 / t32:.4f}")
    shutil.rmtree(tmp, ignore_errors=True)
