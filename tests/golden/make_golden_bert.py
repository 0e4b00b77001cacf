"""Recipe of tests/golden/tiny_bert.npz and tiny_bert_dh128.npz: HF `BertModel` (transformers, CPU, fp32, eager attention) on tiny
random configs -- the reference forward of the BERT family (SGPT_ARCH_BERT), as make_golden.py records HF GPTNeoModel.

    python tests/golden/make_golden_bert.py          (needs torch + transformers; writes next to itself)

Weights: sgpt_amd.model.synthetic_bert_weights(cfg, seed) -- seeded numpy, under HF BertModel state-dict names -- loaded into the HF
module with load_state_dict(strict=True) (the pooler head, which the forward under test ignores, gets zeros).  As the other
tiny_*.npz fixtures do, the file records cfg + seed instead of the ~1.8 MB of fp32 weights (a committed file stays under 1 MiB) plus
a sha256 over the tensors' bytes, so a change of the generator stream fails the reader loudly instead of silently shifting the
expected values.

Inputs: ragged id lists framed [CLS] ... [SEP] (ids 1 / 2; content ids 3 .. vocab - 1), one HF call per sequence (no padding, no
mask arithmetic in the reference values), token types all 0.
  tiny_bert.npz        2 layers, d 128, 2 heads (head_dim 64), ffn 512, vocab 200, max_pos 160;
                       lengths 1, 2, 3, 31, 33, 63, 64, 65, 127, 129: both sides of the 32-row query tile, the 64-key tile and the
                       128-row block of the attention kernel; at length 1 bidirectional == causal
  tiny_bert_dh128.npz  2 layers, d 256, 2 heads (head_dim 128), ffn 512; lengths 5, 64, 130
Recorded: ids (flat) + seq_lens, all L + 1 hidden states per token (flat rows, HF numbering: entry 0 = embedding LayerNorm output),
and the `mean` / `cls` pooled vectors of the last hidden state."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

CLS_ID, SEP_ID = 1, 2
FIXTURES = {
    "tiny_bert": dict(cfg=dict(model_type="bert", vocab_size=200, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                               intermediate_size=512, max_position_embeddings=160, layer_norm_eps=1e-12, type_vocab_size=2,
                               hidden_act="gelu", position_embedding_type="absolute"),
                      lens=[1, 2, 3, 31, 33, 63, 64, 65, 127, 129], seed=11),
    "tiny_bert_dh128": dict(cfg=dict(model_type="bert", vocab_size=200, hidden_size=256, num_hidden_layers=2, num_attention_heads=2,
                                     intermediate_size=512, max_position_embeddings=160, layer_norm_eps=1e-12, type_vocab_size=2,
                                     hidden_act="gelu", position_embedding_type="absolute"),
                            lens=[5, 64, 130], seed=12),
}


def weights_digest(w) -> str:
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def framed_ids(lens, vocab, rng):
    out = []
    for n in lens:
        body = rng.integers(3, vocab, size=max(n - 2, 0)).tolist()
        out.append(([CLS_ID] + body + [SEP_ID])[:n] if n >= 2 else [CLS_ID])
    return out


def main():
    import torch
    from transformers import BertConfig, BertModel
    from sgpt_amd.model import SGPTConfig, synthetic_bert_weights
    for name, fx in FIXTURES.items():
        hf = dict(fx["cfg"])
        cfg = SGPTConfig.from_hf_dict(hf)
        w = synthetic_bert_weights(cfg, seed=fx["seed"])
        bc = BertConfig(**{k: v for k, v in hf.items() if k != "model_type"}, hidden_dropout_prob=0.0,
                        attention_probs_dropout_prob=0.0, attn_implementation="eager")
        model = BertModel(bc, add_pooling_layer=False).eval()
        sd = {k: torch.from_numpy(v) for k, v in w.items()}
        missing = model.load_state_dict(sd, strict=False)
        assert not missing.unexpected_keys and all(k.endswith(("position_ids", "token_type_ids")) for k in missing.missing_keys), missing
        rng = np.random.default_rng(fx["seed"] + 1000)
        seqs = framed_ids(fx["lens"], hf["vocab_size"], rng)
        hidden, mean, cls = [], [], []
        with torch.no_grad():
            for s in seqs:
                out = model(input_ids=torch.tensor([s]), token_type_ids=torch.zeros((1, len(s)), dtype=torch.long),
                            output_hidden_states=True)
                hs = torch.stack(out.hidden_states)[:, 0]            # [L + 1, len, d]
                hidden.append(hs.numpy())
                mean.append(hs[-1].mean(0).numpy())
                cls.append(hs[-1][0].numpy())
        np.savez(os.path.join(HERE, name + ".npz"), cfg=json.dumps(hf), seed=fx["seed"], weights_sha256=weights_digest(w),
                 seq_lens=np.asarray(fx["lens"], np.int64), ids=np.concatenate([np.asarray(s, np.int32) for s in seqs]),
                 hidden=np.concatenate(hidden, axis=1).astype(np.float32), emb_mean=np.stack(mean).astype(np.float32),
                 emb_cls=np.stack(cls).astype(np.float32))
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
