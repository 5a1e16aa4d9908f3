"""Summation error of v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, unit block scales) against float64, the instruction alone: probe_chain of
fp8_mfma_probe.hip chains the accumulator through K / 64 instructions and does nothing else. Operands as tests/_fp8_cases.py draws them: rows
of N(0, 1) scaled so that the row's maximum is 448, rounded to e4m3; K below 64 is zero-padded (what the K-tail mask of csrc/gemm_fp8.hip
feeds). Every product of two e4m3 values and every partial sum of up to 2^15 of them is exact in float64.

Build and run (from this directory):
  hipcc --offload-arch=gfx950 --genco fp8_mfma_probe.hip -o fp8_probe.hsaco && python fp8_mfma_sum_probe.py
Prints one `FP8MFMA` line per K: the worst |D - ref| over `tiles` 32x32 tiles in units of (a) sum_k |a_k b_k| of that element, (b) the
largest |a_k b_k| of that element, (c) the project's F32 tolerance 2e-5 |ref| + 2e-5 rms(ref); and the tiles' relative L2 error."""
import ctypes
import os

import torch

here = os.path.dirname(os.path.abspath(__file__))
hip = ctypes.CDLL("libamdhip64.so")
torch.cuda.init()
torch.zeros(1, device="cuda")
mod = ctypes.c_void_p()
assert hip.hipModuleLoad(ctypes.byref(mod), os.path.join(here, "fp8_probe.hsaco").encode()) == 0
f = ctypes.c_void_p()
assert hip.hipModuleGetFunction(ctypes.byref(f), mod, b"probe_chain") == 0


def chain(A, B, steps):
    Ad, Bd = A.cuda(), B.cuda()
    D = torch.zeros(32, 32, device="cuda")
    args = [ctypes.c_void_p(Ad.data_ptr()), ctypes.c_void_p(Bd.data_ptr()), ctypes.c_void_p(D.data_ptr()), ctypes.c_int(steps)]
    argv = (ctypes.c_void_p * 4)(*[ctypes.cast(ctypes.pointer(a), ctypes.c_void_p) for a in args])
    rc = hip.hipModuleLaunchKernel(f, 1, 1, 1, 64, 1, 1, 0, None, argv, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return D.cpu().double()


def codes(g, K, Kpad):
    x = torch.randn(32, K, generator=g)
    q = (x / x.abs().amax(1, keepdim=True) * 448.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    out = torch.zeros(32, Kpad, dtype=torch.uint8)
    out[:, :K] = q.view(torch.uint8)
    return out.contiguous()


tiles = 48
for K in (16, 64, 80, 128, 144, 320, 336, 2432):
    steps = (K + 63) // 64
    g = torch.Generator().manual_seed(K)
    w_sum = w_max = w_tol = num = den = 0.0
    for _ in range(tiles):
        A, B = codes(g, K, 64 * steps), codes(g, K, 64 * steps)
        a, b = A.view(torch.float8_e4m3fn).double(), B.view(torch.float8_e4m3fn).double()
        ref = a @ b.t()
        prod = (a[:, None, :] * b[None, :, :]).abs()
        err = (chain(A, B, steps) - ref).abs()
        w_sum = max(w_sum, (err / prod.sum(2).clamp_min(1e-30)).max().item())
        w_max = max(w_max, (err / prod.amax(2).clamp_min(1e-30)).max().item())
        w_tol = max(w_tol, (err / (2e-5 * ref.abs() + 2e-5 * ref.pow(2).mean().sqrt())).max().item())
        num, den = num + err.pow(2).sum().item(), den + ref.pow(2).sum().item()
    print(f"FP8MFMA K={K} instructions={steps} tiles={tiles} err/sum|p|={w_sum:.4g} err/max|p|={w_max:.4g} err/F32tol={w_tol:.4g} rel_l2={(num / den) ** 0.5:.4g}", flush=True)
