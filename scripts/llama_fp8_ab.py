#!/usr/bin/env python3
"""Same-process A/B of the Llama family's projections: bf16 (SGPTModel(dtype='bf16')) against fp8 (projections='fp8') on one device,
for profiles/llama_fp8_projections.txt.

Two 4-layer random-init models, at Mistral-7B's shapes (d 4096, 32 / 8 heads of 128, ffn 14336) and at Qwen3-Embedding-0.6B's (d 1024,
16 / 8 heads of 128: query width 2048, key / value width 1024, ffn 3072, head norm); one packed batch of 128 sequences x 512 tokens;
the two arithmetics alternate, five timed windows each (a window = ITERS encode calls between two events, after WARMUP untimed calls).
Printed per shape: the per-call time of every window, mean and spread (max - min) per arithmetic, the ratio bf16 / fp8 with the
spreads beside it, and the bytes of the block weights before and after the conversion.

  timeout -k 10 600 python scripts/llama_fp8_ab.py [OUT]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sgpt_amd import SGPTConfig, SGPTModel  # noqa: E402
from sgpt_amd.families import head_dim  # noqa: E402

N_SEQ, SEQ_LEN, LAYERS, WINDOWS, ITERS, WARMUP = 128, 512, 4, 5, 3, 2
SHAPES = {
    "mistral-7b": dict(hidden_size=4096, num_heads=32, num_kv_heads=8, rotary_dim=0, intermediate_size=14336, qk_norm=False),
    "qwen3-embedding-0.6b": dict(hidden_size=1024, num_heads=16, num_kv_heads=8, rotary_dim=128, intermediate_size=3072, qk_norm=True),
}


def weights(cfg, qk_norm, gen):
    """HF-named random-init tensors on the device (std 0.02; norm gains 1 + 0.1 N(0, 1))."""
    d, ffn, dh = cfg.hidden_size, cfg.intermediate_size, head_dim(cfg)
    dq, dkv = cfg.num_heads * dh, cfg.num_kv_heads * dh

    def nrm(*shape, s=0.02, add=0.0):
        return torch.randn(shape, device="cuda", generator=gen) * s + add
    w = {"embed_tokens.weight": nrm(cfg.vocab_size, d), "norm.weight": nrm(d, s=0.1, add=1.0)}
    for i in range(cfg.num_layers):
        p = f"layers.{i}."
        w[p + "input_layernorm.weight"] = nrm(d, s=0.1, add=1.0)
        w[p + "post_attention_layernorm.weight"] = nrm(d, s=0.1, add=1.0)
        for n, rows in (("q", dq), ("k", dkv), ("v", dkv)):
            w[p + f"self_attn.{n}_proj.weight"] = nrm(rows, d)
        if qk_norm:
            w[p + "self_attn.q_norm.weight"], w[p + "self_attn.k_norm.weight"] = nrm(dh, s=0.1, add=1.0), nrm(dh, s=0.1, add=1.0)
        w[p + "self_attn.o_proj.weight"] = nrm(d, dq)
        w[p + "mlp.gate_proj.weight"], w[p + "mlp.up_proj.weight"], w[p + "mlp.down_proj.weight"] = nrm(ffn, d), nrm(ffn, d), nrm(d, ffn)
    return w


def window(model, pb, out):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        model.encode_packed(pb, mode="mean", normalize=True, out=out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / ITERS


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"llama_fp8_ab: {torch.cuda.get_device_name(0)}; {LAYERS} layers, {N_SEQ} sequences x {SEQ_LEN} tokens = {N_SEQ * SEQ_LEN} rows; "
        f"{WINDOWS} windows of {ITERS} calls per arithmetic, alternating; ms per encode call")
    for name, shape in SHAPES.items():
        shape = dict(shape)
        qk_norm = shape.pop("qk_norm")
        cfg = SGPTConfig(model_type="llama", vocab_size=1024, max_position_embeddings=SEQ_LEN, num_layers=LAYERS, window_size=0, **shape)
        gen = torch.Generator(device="cuda").manual_seed(7)
        w = weights(cfg, qk_norm, gen)
        models = {"bf16": SGPTModel(cfg, w, device="cuda:0", dtype="bf16"), "fp8": SGPTModel(cfg, w, device="cuda:0", dtype="bf16", projections="fp8")}
        del w
        d, ffn, dh = cfg.hidden_size, cfg.intermediate_size, head_dim(cfg)
        dq, dkv = cfg.num_heads * dh, cfg.num_kv_heads * dh
        before = LAYERS * 2 * ((dq + 2 * dkv) * d + d * dq + 2 * ffn * d + d * ffn)
        after = before - models["fp8"].projection_bytes_freed
        ids = torch.randint(0, cfg.vocab_size, (N_SEQ, SEQ_LEN), generator=torch.Generator().manual_seed(3)).numpy()
        pbs = {k: m.pack(ids) for k, m in models.items()}
        outs = {k: torch.empty((N_SEQ, d), device="cuda:0") for k in models}
        for k, m in models.items():
            for _ in range(WARMUP):
                m.encode_packed(pbs[k], mode="mean", normalize=True, out=outs[k])
        torch.cuda.synchronize()
        cos = torch.nn.functional.cosine_similarity(outs["bf16"], outs["fp8"], dim=1)
        t = {k: [] for k in models}
        for _ in range(WINDOWS):
            for k, m in models.items():
                t[k].append(window(m, pbs[k], outs[k]))
        say(f"{name}: d {d}, d_q {dq}, d_kv {dkv}, ffn {ffn}")
        for k in models:
            mean = sum(t[k]) / WINDOWS
            say(f"  {k:5s} windows " + " ".join(f"{v:8.3f}" for v in t[k]) + f"   mean {mean:8.3f}  spread {max(t[k]) - min(t[k]):.3f}")
        mb, mf = sum(t["bf16"]) / WINDOWS, sum(t["fp8"]) / WINDOWS
        say(f"  bf16 / fp8 = {mb / mf:.3f}  (fp8 {'faster' if mf < mb else 'slower'} by {abs(mb - mf):.3f} ms per call; spreads "
            f"{max(t['bf16']) - min(t['bf16']):.3f} / {max(t['fp8']) - min(t['fp8']):.3f} ms)")
        say(f"  block weight bytes: {before} before, {after} after the conversion ({after / before:.3f} of them)")
        say(f"  cosine of the two arithmetics' embeddings (random weights, 128 rows): min {float(cos.min()):.5f}")
        for m in models.values():
            m.close()
        del models, pbs, outs
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
