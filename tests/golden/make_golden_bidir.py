"""Recipe of tests/golden/tiny_*_bidir.npz: HF `LlamaModel` / `Qwen2Model` (transformers, CPU, fp32, eager attention) run BIDIRECTIONALLY on
tiny random configs -- the reference forward of a Llama-family model after sgpt_model_set_attention(0) (SGPTModel(attention=
"bidirectional"): GritLM, gte-Qwen2-instruct, the LLM2Vec checkpoints), as make_golden_llama.py / make_golden_qwen.py record the causal one.

    python tests/golden/make_golden_bidir.py          (needs torch + transformers; writes next to itself)

How the causal mask is switched off: every sequence is one call with `attention_mask = torch.zeros(1, 1, S, S)` -- a 4-D float mask is
taken as the additive mask itself, and all zeros hides nothing.  The recipe ASSERTS that this is what the installed transformers does,
on every sequence of more than one token: row 0 of hidden_states[1] differs from the causal run's (it sees the last token), and row
S - 1 of hidden_states[1] is bit-equal to the causal run's (the last token sees every key either way in the first block).  A version
that ignored the mask would fail the first, one that did anything else to the scores the second: no causal fixture under a
bidirectional name.

Weights: synthetic_llama_weights / synthetic_qwen_weights(cfg, seed) as in the causal recipes (seeds of their own); the file records
cfg + seed and a sha256 over the tensors' bytes instead of the weights (a committed file stays under 1 MiB).

Cases (2 layers, max_position_embeddings 160; `is_causal: false` rides in the recorded config dict, as such checkpoints carry it):
  tiny_llama_bidir         d 128, heads 2 / 1, head_dim 64,  ffn 256     two query heads per key head
  tiny_llama_g4_bidir      d 256, heads 4 / 1, head_dim 64,  ffn 384     four
  tiny_llama_dh128_bidir   d 256, heads 2 / 2, head_dim 128, ffn 384     head_dim 128, no grouping
  tiny_qwen2_bidir         d 128, heads 2 / 1, head_dim 64,  ffn 256     Qwen2Model: the q / k / v bias
Inputs: five sequences of 1, 7, 64, 70 and 130 seeded ids, for make_golden_llama.py's reasons (a single token, odd -- the alignment row
behind it is a key the bidirectional kernel must mask --, exactly one 64-key tile, across a tile, above the 128-row block).
Recorded: ids (flat) + seq_lens, all L + 1 hidden states per token, the mean / weightedmean / lasttoken pooled vectors of the last hidden
state (float64 sums), and the same three pooled from token POOL_FROM = 3 on (`emb_<mode>_from`): rows [min(3, len), len), the weight of
row t still t + 1, the denominator clamped at 1e-9 -- for the 1-token sequence the empty range, a zero row; lasttoken is row len - 1
whatever the range."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)

from make_golden_llama import LENS, weights_digest  # noqa: E402

POOL_FROM = 3


def _cfg(model_type, d, H, kv, ffn, **kw):
    return dict(model_type=model_type, vocab_size=200, hidden_size=d, num_hidden_layers=2, num_attention_heads=H, num_key_value_heads=kv,
                intermediate_size=ffn, max_position_embeddings=160, rope_theta=10000.0, hidden_act="silu", is_causal=False, **kw)


_LLAMA = dict(rms_norm_eps=1e-5, attention_bias=False, mlp_bias=False)
FIXTURES = {
    "tiny_llama_bidir": dict(cfg=_cfg("llama", 128, 2, 1, 256, **_LLAMA), seed=41),
    "tiny_llama_g4_bidir": dict(cfg=_cfg("llama", 256, 4, 1, 384, **_LLAMA), seed=42),
    "tiny_llama_dh128_bidir": dict(cfg=_cfg("llama", 256, 2, 2, 384, **_LLAMA), seed=43),
    "tiny_qwen2_bidir": dict(cfg=_cfg("qwen2", 128, 2, 1, 256, rms_norm_eps=1e-6, use_sliding_window=False), seed=44),
}


def pooled_f64(last: np.ndarray, lo: int) -> dict:
    """mean / weightedmean / lasttoken of one sequence's last hidden state [len, d] over rows [min(lo, len), len), in float64."""
    last = np.asarray(last, dtype=np.float64)
    n = last.shape[0]
    lo = min(max(lo, 0), n)
    w = np.arange(1, n + 1, dtype=np.float64)[lo:]
    rows = last[lo:]
    return {"mean": rows.sum(0) / max(float(n - lo), 1e-9), "weightedmean": (rows * w[:, None]).sum(0) / max(float(w.sum()), 1e-9),
            "lasttoken": last[-1]}


def main():
    import torch
    from transformers import LlamaConfig, LlamaModel, Qwen2Config, Qwen2Model
    from sgpt_amd.model import SGPTConfig, synthetic_llama_weights, synthetic_qwen_weights
    for name, fx in FIXTURES.items():
        hf = dict(fx["cfg"])
        cfg = SGPTConfig.from_hf_dict(hf)
        qwen = hf["model_type"] == "qwen2"
        w = synthetic_qwen_weights(cfg, seed=fx["seed"], qkv_bias=True) if qwen else synthetic_llama_weights(cfg, seed=fx["seed"])
        kw = {k: v for k, v in hf.items() if k not in ("model_type", "is_causal")}
        conf = (Qwen2Config if qwen else LlamaConfig)(**kw, attention_dropout=0.0, attn_implementation="eager")
        model = (Qwen2Model if qwen else LlamaModel)(conf).eval()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        rng = np.random.default_rng(fx["seed"] + 1000)
        seqs = [rng.integers(3, hf["vocab_size"], size=n).tolist() for n in LENS]
        hidden = []
        pooled = {k: [] for k in ("mean", "weightedmean", "lasttoken", "mean_from", "weightedmean_from", "lasttoken_from")}
        with torch.no_grad():
            for s in seqs:
                S, ids = len(s), torch.tensor([s])
                out = model(input_ids=ids, attention_mask=torch.zeros(1, 1, S, S), output_hidden_states=True)
                hs = torch.stack(out.hidden_states)[:, 0]            # [L + 1, len, d]
                assert torch.equal(hs[-1], out.last_hidden_state[0])
                causal = torch.stack(model(input_ids=ids, output_hidden_states=True).hidden_states)[:, 0]
                assert torch.equal(hs[0], causal[0])
                # the zero 4-D mask switched the causal mask off, and did nothing else
                assert torch.equal(hs[1][S - 1], causal[1][S - 1]), "the last token sees every key either way in the first block"
                if S > 1:
                    assert not torch.equal(hs[1][0], causal[1][0]), "row 0 must see the later tokens: this transformers ignores the 4-D mask"
                else:
                    assert torch.equal(hs, causal)
                hidden.append(hs.numpy())
                for sfx, lo in (("", 0), ("_from", POOL_FROM)):
                    for m, v in pooled_f64(hs[-1].numpy(), lo).items():
                        pooled[m + sfx].append(v)
        assert not np.stack(pooled["mean_from"])[0].any() and not np.stack(pooled["weightedmean_from"])[0].any()   # the empty range
        np.savez_compressed(os.path.join(HERE, name + ".npz"), cfg=json.dumps(hf), seed=fx["seed"], qkv_bias=qwen, pool_from=POOL_FROM,
                            weights_sha256=weights_digest(w), seq_lens=np.asarray(LENS, np.int64),
                            ids=np.concatenate([np.asarray(s, np.int32) for s in seqs]),
                            hidden=np.concatenate(hidden, axis=1).astype(np.float32),
                            **{f"emb_{m}": np.stack(v).astype(np.float32) for m, v in pooled.items()})
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
