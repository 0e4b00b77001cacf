"""Shared by the GPU tests of sgpt_linear and sgpt_linear_fp8 (tests/test_gpu_linear_edges.py, tests/test_gpu_linear_256.py,
tests/test_gpu_linear_fp8.py; not a test module): outputs inside guarded buffers of NaN sentinels, the twice-called entry, and the tolerance of a result against the float64 reference of
tests/gemm_ref.py.

Tolerances: `bound` ((K + 4) 2^-23 (|a| |w|^T + |bias| + |resid|), gemm_ref.bound) for fp32 outputs; + u16 |ref| (2^-8 bf16 /
2^-11 f16) for one rounding to a 16-bit output; through a GELU the accumulation bound times 1.13 (max |gelu'|) plus the function's
own allowance -- 2e-3 (bf16) / 5e-4 (f16) absolute for the fast sigmoid form of the 16-bit tanh GELU (tests/test_gpu_linear.py),
2e-5 + 1e-6 |ref| for the fp32 tanh GELU and for the erf GELU in every format (tests/test_gpu_bert.py; the erf epilogue is the
same fp32 code whatever the operand format)."""
import numpy as np
import torch

import gemm_ref as G

DEV = "cuda"
GUARD = 64                                             # elements in front of and behind every output (keeps 16-byte alignment)
SENT32, SENT16 = 0x7FC12345, 0x7FC1                    # NaN bit patterns (fp32; bf16 and f16 alike), compared as integers
SENT8 = 0x7F                                           # the NaN code of e4m3fn: no finite input makes the fp8 epilogue store it
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}
CODE = {"fp32": 0, "bf16": 1, "f16": 3}                # SGPT_F32 / SGPT_BF16 / SGPT_F16


def _sentinel(ity):
    return {torch.int32: SENT32, torch.int16: SENT16, torch.uint8: SENT8}[ity]


def guarded(n, out_t, init=None):
    """[GUARD | n elements | GUARD] as integers, everything the sentinel; the middle also as a view of the output type (fp32, a
    16-bit float, or uint8 for e4m3 codes)."""
    ity = torch.int32 if out_t == torch.float32 else torch.uint8 if out_t == torch.uint8 else torch.int16
    sent = _sentinel(ity)
    buf = torch.full((n + 2 * GUARD,), sent, dtype=ity, device=DEV)
    body = buf[GUARD:GUARD + n].view(out_t)
    if init is not None:
        body.copy_(init.reshape(-1))
    return buf, body


def check_guards(buf, n, what):
    sent = _sentinel(buf.dtype)
    assert bool((buf[:GUARD] == sent).all()), f"{what}: a store in front of the output"
    assert bool((buf[GUARD + n:] == sent).all()), f"{what}: a store behind the output"
    assert not bool((buf[GUARD:GUARD + n] == sent).any()), f"{what}: an element of the output was left unwritten"


def run(ctx, dtype, epi, out16, a_d, w_d, bias_d, resid_d, inplace=False, what=""):
    """sgpt_linear into guarded buffers, twice; guards, no sentinel left, finite, same bits.  Returns the output (device)."""
    (M, K), N = a_d.shape, w_d.shape[0]
    out_t = TORCH[dtype] if out16 else torch.float32
    bufs = []
    for _ in range(2):
        buf, body = guarded(M * N, out_t, init=resid_d if (epi == 2 and inplace) else None)
        resid_p = None if epi != 2 else (body.data_ptr() if inplace else resid_d.data_ptr())
        st = ctx.lib.sgpt_linear(ctx.handle, CODE[dtype], epi, CODE[dtype] if out16 else 0, a_d.data_ptr(), w_d.data_ptr(),
                                 None if bias_d is None else bias_d.data_ptr(), resid_p, body.data_ptr(), M, N, K, None)
        ctx._chk(st, f"sgpt_linear {what}")
        check_guards(buf, M * N, what)
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]), f"{what}: two identical calls, different bits"
    out = body.view((N, M) if epi == 4 else (M, N))
    assert bool(torch.isfinite(out).all()), f"{what}: not finite"
    return out


def tolerance(dtype, epi, out16, ref, bnd):
    """See the module docstring.  ref, bnd: float64 arrays of the output's shape."""
    if epi in (1, 9):
        tol = G.GELU_SLOPE * bnd
        if epi == 1 and dtype != "fp32":
            tol = tol + (2e-3 if dtype == "bf16" else 5e-4)
        else:
            tol = tol + 2e-5 + 1e-6 * np.abs(ref)
    else:
        tol = bnd
    if out16:
        tol = tol + G.U16[dtype] * np.abs(ref)
    return tol
