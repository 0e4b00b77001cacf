#!/usr/bin/env python3
"""Same-process A/B of two builds of the library on the row kernels of csrc/elementwise.hip: parent A / new / parent B, three contexts
in ONE process (ctx_for and the timing loop `ab` of scripts/score_tile_ab.py; parent B is a COPY of the parent's library file, so
|A - B| holds what a context alone moves).  Every output of the two builds must be torch.equal before a case is timed, and, untimed, at
T = 5 over every width rung (tests/rowops_ref.py::LN_WIDTHS) for the five norm kernels in every output format.  Timed shapes: the ones
the project's benchmarks run (bench.py's headline: 131 072 token rows of d = 768; scripts/bert_bench.py; scripts/llama_bench.py: d = 4096,
32 / 8 heads of 128; the bloom-7b1 fp8 configuration; a 1 M x 768 corpus).  Criterion per case: |new - mean(A, B)| <= |A - B|, or faster.

  SGPT_LIB_TAG=parent python -m sgpt_amd.build      # at the parent commit; then copy libsgpt_hip_parent.so to a second name
  python scripts/rowops_ab.py PARENT_LIB NEW_LIB OUT PARENT_LIB_COPY"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

from rowops_ref import LN_WIDTHS  # noqa: E402
from score_tile_ab import ab, ctx_for  # noqa: E402
from sgpt_amd.families import rotary_tables_half  # noqa: E402
from sgpt_amd.runtime import DT_CODE, _p, _stream_ptr  # noqa: E402

EPS = 1e-5
HALVES = (torch.float16, torch.bfloat16)
compared = 0


def same(what, a, b):
    """a, b: the outputs (lists of tensors) of the parent's and the new build."""
    global compared
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and torch.equal(u.view(torch.uint8), v.view(torch.uint8)), f"{what}: output {i} differs between the builds"
        compared += 1


def rand(gen, *shape, mul=1.0, add=0.0):
    return torch.randn(shape, device="cuda", generator=gen) * mul + add


def writeback(ctx, x, g, b, out16):
    ctx._chk(ctx.lib.sgpt_layernorm_writeback(ctx.handle, _p(x), _p(g), _p(b), x.shape[0], x.shape[1], EPS, _p(out16), DT_CODE[out16.dtype],
                                              _stream_ptr(ctx.device)), "sgpt_layernorm_writeback")


def layernorm_fp8(ctx, x, g, b, codes, scale):
    ctx._chk(ctx.lib.sgpt_layernorm_fp8(ctx.handle, _p(x), _p(g), _p(b), x.shape[0], x.shape[1], EPS, _p(codes), _p(scale),
                                        _stream_ptr(ctx.device)), "sgpt_layernorm_fp8")


def fp8_quantize(ctx, w, codes, scale):
    ctx._chk(ctx.lib.sgpt_fp8_quantize_rows(ctx.handle, _p(w), w.shape[0], w.shape[1], _p(codes), _p(scale), _stream_ptr(ctx.device)),
             "sgpt_fp8_quantize_rows")


def norm_outputs(ctx, x, g, b):
    """Every output format of the five norm kernels on one input."""
    T, d = x.shape
    outs = [ctx.layernorm(x, g, b, EPS)]
    xin = x.clone()
    outs.append(ctx.layernorm(xin, g, b, EPS, out=xin))
    for h, mul in ((torch.bfloat16, 1.0), (torch.float16, 1.0), (torch.float16, 0.125)):
        outs.append(ctx.layernorm(x, g, b, EPS, out_dtype=h, out_mul=mul))
        outs.append(ctx.layernorm(x, g, b, EPS, out_dtype=h, out_mul=mul, split=True))
    for h in HALVES:
        xin, o16 = x.clone(), torch.empty((T, d), dtype=h, device="cuda")
        writeback(ctx, xin, g, b, o16)
        outs += [xin, o16]
    outs += [ctx.rmsnorm(x, g, EPS, out_dtype=t) for t in (torch.float32,) + HALVES]
    xin = x.clone()
    outs.append(ctx.rmsnorm(xin, g, EPS, out=xin))
    codes, scale = torch.empty((T, d), dtype=torch.uint8, device="cuda"), torch.empty((T,), dtype=torch.float32, device="cuda")
    layernorm_fp8(ctx, x, g, b, codes, scale)
    return outs + [codes, scale]


def main():
    parent_lib, new_lib, out, parent_copy = sys.argv[1:5]
    ctxs = [ctx_for(parent_lib), ctx_for(new_lib), ctx_for(parent_copy)]             # parent A, new, parent B
    lines = [f"# parent = {os.path.basename(parent_lib)}, new = {os.path.basename(new_lib)}; one process, parent B = a second instance of the "
             "parent library (its own context); order per repeat: parent A, new, parent B; median of 7 windows (min .. max)"]
    print(lines[0], flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)

    for d in LN_WIDTHS:
        x, g, b = rand(gen, 5, d, mul=3.0, add=0.5), rand(gen, d, mul=0.1, add=1.0), rand(gen, d, mul=0.1)
        pa, nw = norm_outputs(ctxs[0], x, g, b), norm_outputs(ctxs[1], x, g, b)
        same(f"T=5 d={d}", pa, nw)
    lines.append(f"# T = 5, d in {LN_WIDTHS}: {compared} outputs of the five norm kernels bit-identical between the builds")
    print(lines[-1], flush=True)

    def case(name, make):
        """make(ctx) -> (run, outputs): run is one timed pass on buffers of the context's own, outputs() what it left behind."""
        made = [make(c) for c in ctxs]
        for run, _ in made:
            run()
        same(name, made[0][1](), made[1][1]())
        same(name + " (parent B)", made[0][1](), made[2][1]())
        ab(name, made[0][0], made[1][0], lines, made[2][0])

    T = 131072
    for d, cases in ((768, ("layernorm f16", "layernorm fp32 in place", "layernorm split f16", "write-back f16")),
                     (4096, ("rmsnorm bf16", "layernorm fp8"))):
        x, g, b = rand(gen, T, d, mul=3.0, add=0.5), rand(gen, d, mul=0.1, add=1.0), rand(gen, d, mul=0.1)

        def make(ctx, what):
            if what == "layernorm f16":
                o = torch.empty((T, d), dtype=torch.float16, device="cuda")
                return (lambda: ctx.layernorm(x, g, b, EPS, out_dtype=torch.float16, out=o)), (lambda: [o])
            if what == "layernorm split f16":
                o = torch.empty((T, 3 * d), dtype=torch.float16, device="cuda")
                return (lambda: ctx.layernorm(x, g, b, EPS, out_dtype=torch.float16, split=True, out=o)), (lambda: [o])
            if what == "rmsnorm bf16":
                o = torch.empty((T, d), dtype=torch.bfloat16, device="cuda")
                return (lambda: ctx.rmsnorm(x, g, EPS, out_dtype=torch.bfloat16, out=o)), (lambda: [o])
            if what == "layernorm fp8":
                codes, scale = torch.empty((T, d), dtype=torch.uint8, device="cuda"), torch.empty((T,), dtype=torch.float32, device="cuda")
                return (lambda: layernorm_fp8(ctx, x, g, b, codes, scale)), (lambda: [codes, scale])
            xin = x.clone()                      # in place: every pass normalises the rows the one before left, the same in every context
            if what == "layernorm fp32 in place":
                return (lambda: ctx.layernorm(xin, g, b, EPS, out=xin)), (lambda: [xin])
            o16 = torch.empty((T, d), dtype=torch.float16, device="cuda")
            return (lambda: writeback(ctx, xin, g, b, o16)), (lambda: [xin, o16])
        for what in cases:
            case(f"{what} {T} x {d}", lambda ctx: make(ctx, what))
        del x

    d = 768
    for B, S in ((1024, 128), (1, 30)):
        x, g, b = rand(gen, B * S, d, mul=2.0, add=0.3), rand(gen, d, mul=0.1, add=1.0), rand(gen, d, mul=0.1)
        off = torch.arange(B + 1, dtype=torch.int32, device="cuda") * S
        ln = torch.full((B,), S, dtype=torch.int32, device="cuda")
        keep = {}

        def make(ctx):
            def run():
                keep[ctx] = ctx.lnf_pool(x, off, ln, ln=(g, b, EPS), mode="weightedmean", normalize=True)
            return run, (lambda: [keep[ctx]])
        case(f"lnf_pool {B} sequences of {S} tokens, d = {d}", make)

    T, H, Hkv, dh = 32768, 32, 8, 128
    ld = (H + 2 * Hkv) * dh
    sin, cos = (torch.from_numpy(t).to("cuda") for t in rotary_tables_half(2048, dh))
    pos = (torch.arange(T, dtype=torch.int32, device="cuda") % 128).contiguous()
    buf0 = rand(gen, T, ld).to(torch.bfloat16)
    qg, kg = rand(gen, dh, mul=0.1, add=1.0), rand(gen, dh, mul=0.1, add=1.0)

    def make_rope(ctx):
        buf = buf0.clone()                       # in place, as above
        return (lambda: ctx.rope_half(buf, pos, sin, cos, H, Hkv, dh, k_off=H * dh)), (lambda: [buf])

    def make_qknorm(ctx):
        buf = buf0.clone()
        return (lambda: ctx.qknorm_rope_half(buf, pos, sin, cos, qg, kg, H, Hkv, dh, k_off=H * dh, eps=1e-6)), (lambda: [buf])
    case(f"rope_half {T} tokens, H = {H}, H_kv = {Hkv}, dh = {dh}, bf16", make_rope)
    case(f"qknorm_rope_half {T} tokens, H = {H}, H_kv = {Hkv}, dh = {dh}, bf16", make_qknorm)
    del buf0

    w = torch.nn.functional.normalize(rand(gen, 1_000_000, 768), dim=1)

    def make_quant(ctx):
        codes, scale = torch.empty(w.shape, dtype=torch.uint8, device="cuda"), torch.empty((w.shape[0],), dtype=torch.float32, device="cuda")
        return (lambda: fp8_quantize(ctx, w, codes, scale)), (lambda: [codes, scale])
    case("fp8_quantize_rows 1 000 000 x 768", make_quant)

    lines.append(f"# {compared} output comparisons in all, every one bit-identical")
    print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
