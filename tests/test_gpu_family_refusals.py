"""What each model family refuses through the C ABI, and what it serves: status and the exact sgpt_last_error text.

One tiny model per SGPT_ARCH_* value (one layer, d_model 128, two heads of 64, d_ffn 128), loaded through sgpt_model_load itself -- the
Python host refuses most of these calls before they reach the library.  The expected strings are literals taken from the sources
as they stood before the families were given one table in the host code: they pin the ABI's behaviour, not the table."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sgpt_oracle as O

pytestmark = pytest.mark.gpu

INVALID, MISSING = -1, -3
V, P, D, H, FFN = 40, 64, 128, 2, 128
NEO, GPTJ, BLOOM, BERT, LLAMA = 0, 1, 2, 3, 4
ARCHES = (NEO, GPTJ, BLOOM, BERT, LLAMA)
DECODERS = (NEO, GPTJ, BLOOM)
NAME = {BERT: "SGPT_ARCH_BERT", LLAMA: "SGPT_ARCH_LLAMA"}
F32, BF16, FP8W, F16, FP8M = 0, 1, 2, 3, 4
PC_ATT, PC_CTX = 1, 2

E_FP8 = "%s: compute_dtype SGPT_F32, SGPT_F16 or SGPT_BF16 (no fp8 mode for this family)"
E_SPLIT = "%s: qk_split / split_weights (split-precision operands) are not available for this family"
E_DH16 = "16-bit attention supports head_dim 64, 128 or 256"
E_DH_BERT = "SGPT_ARCH_BERT: 16-bit bidirectional attention supports head_dim 64 or 128"
E_DH_LLAMA = "SGPT_ARCH_LLAMA: head_dim 64 or 128"
E_WIN_BERT = "SGPT_ARCH_BERT: window must be 0"
E_WIN_LLAMA = "SGPT_ARCH_LLAMA: window >= 0"
E_NKV = "n_kv_heads (grouped K / V) belongs to SGPT_ARCH_LLAMA"
E_NKV_LLAMA = "SGPT_ARCH_LLAMA: n_heads % n_kv_heads == 0 (0 = n_heads)"
E_ADAPT = ("sgpt_model_range_adapt: SGPT_ARCH_BERT / SGPT_ARCH_LLAMA run without range shifts; a flagged f16 model must be loaded with "
           "SGPT_BF16 or SGPT_F32")
E_ADAPT_DTYPE = "sgpt_model_range_adapt applies to SGPT_F16 models"
E_SHIFTS = "sgpt_model_set_range_shifts: SGPT_ARCH_BERT / SGPT_ARCH_LLAMA run without range shifts"
E_PREC = "sgpt_model_set_precision: no split-precision operands for SGPT_ARCH_BERT / SGPT_ARCH_LLAMA"
E_PREC_COPIES = "sgpt_model_set_precision: the model was loaded without split weight copies (sgpt_model_desc.split_weights)"
E_PREC_ROTARY = "sgpt_model_set_precision: split-precision attention needs head_dim 64 or 128 and no rotary embedding (GPT-Neo / BLOOM)"
E_PROBE = "the precision probe applies to SGPT_F16 / SGPT_BF16 models of the decoder families"
E_LEARNT = "sgpt_encode: learntmean pooling (trained position weights of the SGPT checkpoints) is not available for %s"
E_LEARNT_TABLE = "sgpt_encode: learntmean needs sgpt_model_set_pool_weights first"
E_CLS = "sgpt_encode: cls pooling belongs to SGPT_ARCH_BERT"
E_LM = {BERT: "sgpt_lm_logprobs: SGPT_ARCH_BERT carries no causal LM head",
        LLAMA: "sgpt_lm_logprobs: not built for SGPT_ARCH_LLAMA (the LM head of this family is not loaded)"}


def family_weights(arch, n_kv=H):
    """Seeded weights of the tiny model under the tensor names include/sgpt_hip.h asks for."""
    from sgpt_amd import model as M
    kw = dict(vocab_size=V, max_position_embeddings=P, hidden_size=D, num_layers=1, num_heads=H, intermediate_size=FFN, window_size=8)
    if arch == NEO:
        return M.synthetic_weights(M.SGPTConfig(**kw), seed=3)
    if arch == GPTJ:
        w = O.synth_weights_gptj(O.GPTJConfig(vocab_size=V, n_positions=P, n_embd=D, n_layer=1, n_head=H, rotary_dim=32, n_inner=FFN), seed=3)
        w["rotary.sin"], w["rotary.cos"] = M.rotary_tables(P, 32)
        return w
    if arch == BLOOM:
        cfg = O.BloomConfig(vocab_size=V, hidden_size=D, n_layer=1, n_head=H)
        cfg.intermediate_size = FFN
        w = O.synth_weights_bloom(cfg, seed=3)
        w["alibi.slopes"] = M.alibi_slopes(H)
        return w
    if arch == BERT:
        return M.bert_state_dict(M.synthetic_bert_weights(M.SGPTConfig(model_type="bert", **kw), seed=3))
    w = M.llama_state_dict(M.synthetic_llama_weights(M.SGPTConfig(model_type="llama", num_kv_heads=n_kv, **kw), seed=3))
    w["rotary.sin"], w["rotary.cos"] = M.rotary_tables_half(P, D // H)
    return w


class Lib:
    """The library and one context, plus the tiny models: loaded once, freed at the end of the module."""

    def __init__(self):
        from sgpt_amd import _lib, get_context
        self.L = _lib
        self.ctx = get_context("cuda:0")
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.tensors, self.models = {}, {}

    def err(self):
        return (self.lib.sgpt_last_error(self.h) or b"").decode()

    def load(self, arch, dtype, real=True, n_kv=0, **over):
        """sgpt_model_load -> (status, handle).  real=False: one dummy tensor (the descriptor is judged before any tensor is read)."""
        key = (arch, n_kv or H)
        if real and key not in self.tensors:
            self.tensors[key] = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to("cuda:0", torch.float32).contiguous()
                                 for k, v in family_weights(arch, n_kv or H).items()}
        t = self.tensors[key] if real else {}
        views = (self.L.TensorView * max(1, len(t)))(*[self.L.TensorView(k.encode(), v.data_ptr(), v.numel()) for k, v in t.items()])
        d = dict(arch=arch, n_layers=1, d_model=D, n_heads=H, d_ffn=FFN, vocab=V, max_pos=P, window=0 if arch == BERT else 8, ln_eps=1e-5,
                 attn_scale=1.0 if arch == NEO else 0.125, compute_dtype=dtype, rotary_dim=32 if arch == GPTJ else 0, qk_split=0, split_weights=0,
                 n_kv_heads=n_kv)
        d.update(over)
        desc = self.L.ModelDesc(**d)
        hh = C.c_void_p()
        torch.cuda.synchronize()
        st = self.lib.sgpt_model_load(self.h, C.byref(desc), views, len(t), C.byref(hh))
        assert (st == 0) == bool(hh.value)
        return st, hh

    def model(self, arch, dtype, **over):
        key = (arch, dtype) + tuple(sorted(over.items()))
        if key not in self.models:
            st, hh = self.load(arch, dtype, **over)
            assert st == 0, (arch, dtype, over, self.err())
            self.models[key] = hh
        return self.models[key]

    def close(self):
        for hh in self.models.values():
            self.lib.sgpt_model_free(hh)


@pytest.fixture(scope="module")
def g():
    lib = Lib()
    yield lib
    lib.close()


def refused(g, st, text, status=INVALID):
    assert st == status and g.err() == text, (st, g.err())


def test_load_fp8_and_split_operands(g):
    for arch in (BERT, LLAMA):
        for dt in (FP8W, FP8M):
            refused(g, g.load(arch, dt, real=False)[0], E_FP8 % NAME[arch])
        for kw in (dict(qk_split=1), dict(split_weights=1)):
            refused(g, g.load(arch, F16, real=False, **kw)[0], E_SPLIT % NAME[arch])
        refused(g, g.load(arch, FP8W, real=False, window=-1, n_kv_heads=3)[0], E_FP8 % NAME[arch])     # the first rule broken answers
    for arch in DECODERS:
        for dt, kw in ((FP8W, {}), (FP8M, {}), (F16, dict(qk_split=1)), (BF16, dict(split_weights=1))):
            g.model(arch, dt, **kw)


def test_load_head_dim(g):
    for arch in ARCHES:
        for dt in (F16, BF16):
            refused(g, g.load(arch, dt, real=False, n_heads=4)[0], E_DH16)                             # head_dim 32
    refused(g, g.load(BERT, F16, real=False, d_model=256, n_heads=1)[0], E_DH_BERT)                    # head_dim 256
    for dt in (F16, F32):
        refused(g, g.load(LLAMA, dt, real=False, d_model=256, n_heads=1)[0], E_DH_LLAMA)
    refused(g, g.load(LLAMA, F32, real=False, n_heads=4)[0], E_DH_LLAMA)
    refused(g, g.load(LLAMA, F32, real=False, d_model=384, n_heads=2)[0], E_DH_LLAMA)                  # head_dim 192
    refused(g, g.load(BERT, F32, real=False, n_heads=4)[0], "missing weight tensor: embeddings.LayerNorm.bias", MISSING)   # fp32 serves it: on to the tensors


def test_load_window_and_kv_heads(g):
    refused(g, g.load(BERT, F16, real=False, window=8)[0], E_WIN_BERT)
    refused(g, g.load(BERT, F16, real=False, window=8, n_kv_heads=1)[0], E_WIN_BERT)
    refused(g, g.load(LLAMA, F16, real=False, window=-1)[0], E_WIN_LLAMA)
    refused(g, g.load(LLAMA, F16, real=False, window=-1, n_kv_heads=3)[0], E_NKV_LLAMA)
    refused(g, g.load(LLAMA, F16, real=False, n_kv_heads=-1)[0], E_NKV_LLAMA)
    for arch in (NEO, GPTJ, BLOOM, BERT):
        refused(g, g.load(arch, F16, real=False, n_kv_heads=1)[0], E_NKV)
        g.model(arch, F16, n_kv=H)                      # n_kv_heads = n_heads says nothing new: accepted; a window too (BERT: 0)
    g.model(LLAMA, F16, n_kv=1)                         # grouped K / V is this family's
    g.model(LLAMA, F16, window=0)


def test_range_shifts(g):
    n, zeros = C.c_int32(7), np.zeros(4, dtype=np.int32)
    for arch in ARCHES:
        refused(g, g.lib.sgpt_model_range_adapt(g.model(arch, BF16), C.byref(n), None), E_ADAPT_DTYPE)
        m = g.model(arch, F16)
        adapt = g.lib.sgpt_model_range_adapt(m, C.byref(n), None)
        if arch in DECODERS:
            assert adapt == 0 and n.value == 0, (arch, g.err())
            assert g.lib.sgpt_model_set_range_shifts(m, zeros.ctypes.data_as(C.c_void_p), 4) == 0, (arch, g.err())
        else:
            refused(g, adapt, E_ADAPT)
            refused(g, g.lib.sgpt_model_set_range_shifts(m, zeros.ctypes.data_as(C.c_void_p), 4), E_SHIFTS)


def test_precision_plan_and_probe(g):
    def set_plan(m, cls):
        plan = np.zeros(5, dtype=np.int32)
        if cls is not None:
            plan[cls] = 1
        return g.lib.sgpt_model_set_precision(m, plan.ctypes.data_as(C.c_void_p), 5)

    for arch in ARCHES:
        for dt in (F16, BF16):
            m = g.model(arch, dt)
            refused(g, set_plan(m, PC_CTX), E_PREC_COPIES)        # no family here has split copies: that rule answers first
            st = set_plan(m, PC_ATT)                              # the attention class splits activations only
            if arch in (BERT, LLAMA):
                refused(g, st, E_PREC)
                refused(g, g.lib.sgpt_model_precision_probe_begin(m), E_PROBE)
            elif arch == GPTJ:
                refused(g, st, E_PREC_ROTARY)
            else:
                assert st == 0 and set_plan(m, None) == 0, (arch, g.err())
            assert set_plan(m, None) == 0                         # the all-plain plan is every family's
            if arch in DECODERS:
                assert g.lib.sgpt_model_precision_probe_begin(m) == 0 and g.lib.sgpt_model_precision_probe_end(m, None) == 0, (arch, g.err())
    for arch in DECODERS:
        m = g.model(arch, BF16, split_weights=1)
        assert set_plan(m, PC_CTX) == 0 and set_plan(m, None) == 0, (arch, g.err())


def test_pooling_modes_and_lm_head(g):
    from sgpt_amd.model import pack_host
    pb = pack_host([[1, 2, 3, 4, 5], [6, 7, 8]])
    dev = {k: torch.from_numpy(np.ascontiguousarray(pb[k])).cuda() for k in ("ids", "pos", "seq_off", "seq_len")}
    out = torch.zeros((pb["B"], D), device="cuda")
    hidden = torch.zeros((pb["T_pad"], D), device="cuda")
    idx = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    lp = torch.zeros(2, device="cuda")
    pool_w = torch.ones(P, device="cuda")

    def encode(m, mode):
        return g.lib.sgpt_encode(m, dev["ids"].data_ptr(), dev["pos"].data_ptr(), dev["seq_off"].data_ptr(), dev["seq_len"].data_ptr(), None,
                                 pb["B"], pb["T_pad"], pb["max_alloc"], mode, 1, 1, 0, out.data_ptr(), None, None)

    for arch in ARCHES:
        for dt in (F16, BF16):
            m = g.model(arch, dt)
            if arch in DECODERS:
                refused(g, encode(m, 3), E_LEARNT_TABLE, MISSING)
                assert g.lib.sgpt_model_set_pool_weights(m, pool_w.data_ptr(), P) == 0 and encode(m, 3) == 0, (arch, g.err())
            else:
                refused(g, encode(m, 3), E_LEARNT % NAME[arch])
            if arch == LLAMA:
                refused(g, encode(m, 4), E_CLS)
            else:
                assert encode(m, 4) == 0, (arch, g.err())
            st = g.lib.sgpt_lm_logprobs(m, hidden.data_ptr(), idx.data_ptr(), idx.data_ptr(), 2, lp.data_ptr(), None, None)
            if arch in DECODERS:
                assert st == 0, (arch, g.err())
            else:
                refused(g, st, E_LM[arch])
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(lp).all()
