"""What long sequences cost: one sgpt_encode call over the SAME 32 768 token rows cut into 16 x 2048, 4 x 8192 and 1 x 32 768 tokens, at
Qwen3-Embedding-0.6B shape (28 layers, d 1024, 16 query / 8 key-value heads of 128, ffn 3072, q / k head norm) in bf16.

    python scripts/long_seq_bench.py [--rounds 5] [--iters 3] [--out profiles/long_sequences.txt]

The projections, norms and the MLP see 32 768 rows in every case; what changes is the causal attention: the key tiles a query walks grow
with its position, 2048 / 2 keys per query on average in the first case and 32 768 / 2 in the last (16 x the attention work), and the
blocks of one (sequence, head) that share a K / V^T staging.  No bar is attached: the file records the cost on this design.

Method: random-init weights (ONE layer's tensors handed to all 28 layers, as scripts/llama_bench.py: the rate does not depend on the
values), `lasttoken` pooling, normalised.  Every shape is warmed up (2 calls); then `rounds` rounds, each timing `iters` back-to-back
calls per shape between two device events with one synchronisation, the shapes in ALTERNATING order from round to round (forward, then
reversed) so that a drift of the box lands on all of them.  Reported: the median over rounds of ms per call, the min .. max spread, and
tokens/s from the median.  The results must not depend on the cut more than the arithmetic says: the 2048-token sequences are prefixes of
the 8192-token ones of the 32 768-token one, and the script checks that the first sequence's embedding is finite in every case."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sgpt_amd import SGPTConfig, SGPTModel  # noqa: E402
from sgpt_amd.model import synthetic_qwen_weights  # noqa: E402

ROWS = 32768
CUTS = (2048, 8192, 32768)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "long_seq_bench measures on the GPU: no device, no number"
    hf = dict(model_type="qwen3", vocab_size=151669, hidden_size=1024, num_hidden_layers=a.layers, num_attention_heads=16,
              num_key_value_heads=8, head_dim=128, intermediate_size=3072, max_position_embeddings=32768, rms_norm_eps=1e-6,
              rope_theta=1000000.0, hidden_act="silu", attention_bias=False, use_sliding_window=False, sliding_window=None)
    cfg = SGPTConfig.from_hf_dict(hf)
    one = synthetic_qwen_weights(SGPTConfig.from_hf_dict(dict(hf, num_hidden_layers=1)), 0, qk_norm=True)
    w = {k: v for k, v in one.items() if not k.startswith("layers.")}
    for i in range(cfg.num_layers):
        w.update({k.replace("layers.0.", f"layers.{i}."): v for k, v in one.items() if k.startswith("layers.0.")})
    m = SGPTModel(cfg, w, device="cuda:0", dtype="bf16")
    del w, one
    ids = np.random.default_rng(0).integers(3, hf["vocab_size"], size=ROWS)
    packed, outs = {}, {}
    for n in CUTS:
        packed[n] = m.pack([ids[i:i + n].tolist() for i in range(0, ROWS, n)])
        assert packed[n].T_pad == ROWS and packed[n].max_alloc == n
        outs[n] = torch.empty((ROWS // n, cfg.hidden_size), dtype=torch.float32, device=m.device)

    def call(n):
        m.encode_packed(packed[n], mode="lasttoken", normalize=True, out=outs[n])

    for n in CUTS:
        for _ in range(2):
            call(n)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(outs[n]).all()) for n in CUTS) and m.range_flags() == 0
    times = {n: [] for n in CUTS}
    for r in range(a.rounds):
        for n in (CUTS if r % 2 == 0 else CUTS[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                call(n)
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) / a.iters)
    lines = [f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}",
             f"command: python scripts/long_seq_bench.py --rounds {a.rounds} --iters {a.iters} --layers {a.layers}",
             f"model: Qwen3-Embedding-0.6B shape, random-init, bf16, {cfg.num_layers} layers; one sgpt_encode call of {ROWS} token rows, lasttoken",
             "sequences x tokens      ms per call (median)   min .. max over rounds    tokens/s (median)"]
    for n in CUTS:
        med = statistics.median(times[n])
        lines.append(f"{ROWS // n:>9} x {n:<6}      {med:>12.2f}           {min(times[n]):>8.2f} .. {max(times[n]):<8.2f}      {ROWS / med * 1e3:>12.0f}")
        print(json.dumps(dict(sequences=ROWS // n, tokens=n, ms_per_call=round(med, 3), ms_min=round(min(times[n]), 3),
                              ms_max=round(max(times[n]), 3), tokens_per_s=round(ROWS / med * 1e3, 1), rounds=a.rounds, iters=a.iters)), flush=True)
    base = statistics.median(times[CUTS[0]])
    lines.append("over the 16 x 2048 call: " + ", ".join(f"{ROWS // n} x {n}: {statistics.median(times[n]) / base:.2f}x" for n in CUTS[1:]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    m.close()


if __name__ == "__main__":
    main()
