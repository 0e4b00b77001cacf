"""What the Python layer hands to the C ABI for every corpus kind, pinned without a device or the library: a Context whose `lib` records
each entry's name and arguments (ints and floats as they are, pointers as "null" / "ptr") and returns SGPT_OK.  The C calls do nothing,
so built codes are uninitialised memory: the uint8 builds get `ranges=` (nothing reads the codes back), and only call records are
asserted, never values.  d = 44 is padded by every kind (fp8 to 48 columns, bits to ldb = 8, uint8 to ld = 128) and nq = 70 is more
than one uint8 query group.  The expected records are those of the commit before corpus.py existed, except where a test says otherwise."""
import ctypes as C

import pytest
import torch

N, D, NQ, K, BASE = 300, 44, 70, 10, 5


def _show(a):
    if isinstance(a, (int, float)):
        return a
    if a is None or (isinstance(a, C.c_void_p) and not a.value):
        return "null"
    return "ptr"                    # a c_void_p with an address, or C.byref(...)


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name,) + tuple(_show(a) for a in args))
            return 0
        return entry


@pytest.fixture
def ctx(monkeypatch):
    import sgpt_amd.runtime as RT
    import sgpt_amd.util as U
    c = RT.Context.__new__(RT.Context)
    c.device, c.handle, c.lib = torch.device("cpu"), None, Recorder()
    monkeypatch.setattr(RT, "_stream_ptr", lambda device: None)
    monkeypatch.setattr(RT, "get_context", lambda device=None: c)
    monkeypatch.setattr(U, "get_context", lambda device=None: c)
    return c


def _corpora(ctx):
    emb = torch.zeros(N, D)
    ranges = torch.stack([-torch.ones(D), torch.ones(D)])
    out = {"rows": emb,
           "fp8": ctx.quantize_corpus(emb),
           "uint8": ctx.scalar_quantize_corpus(emb, ranges=ranges),
           "bits": ctx.binarize_corpus(emb, keep_fp8=True, keep_uint8=True, ranges=ranges),
           "bits_centred": ctx.binarize_corpus(emb, center=torch.zeros(D), keep_uint8=True, ranges=ranges)}
    ctx.lib.calls.clear()
    return out


def _run():
    return torch.empty(NQ, K), torch.empty(NQ, K, dtype=torch.int64), 3


# case -> (corpus, keywords of score_topk)
SCORE_CASES = {
    "rows": ("rows", {}),
    "fp8": ("fp8", {}),
    "uint8": ("uint8", {}),
    "bits none": ("bits", {"rescore": "none"}),
    "bits sign": ("bits", {"rescore": "sign"}),
    "bits fp8": ("bits", {"rescore": "fp8"}),
    "bits uint8": ("bits", {"rescore": "uint8"}),
    "bits_centred uint8": ("bits_centred", {"rescore": "uint8"}),
}

# the calls of score_topk(q [70, 44], corpus, 10, idx_base=5): fresh, n_run = 0; with run=, n_run = 3 -- nothing else differs
TO_F16 = ("sgpt_f32_to_16", "null", "ptr", NQ * 48, "ptr", 3, "null")
SCORE_EXPECTED = {
    "rows": lambda n_run, base=BASE: [("sgpt_score_topk", "null", "ptr", "ptr", 0, 70, 300, 44, 10, base, "ptr", "ptr", n_run, "ptr", "null")],
    "fp8": lambda n_run, base=BASE: [TO_F16, ("sgpt_score_topk_q8", "null", "ptr", "ptr", "ptr", 70, 300, 48, 10, base, "ptr", "ptr", n_run, "ptr", "null")],
    "uint8": lambda n_run, base=BASE: [("sgpt_score_topk_u8", "null", "ptr", "ptr", "ptr", "ptr", nq, 300, 44, 128, 10, base, "ptr", "ptr", n_run, "ptr", "null")
                            for nq in (64, 6)],
    "bits none": lambda n_run, base=BASE: [("sgpt_score_topk_bits", "null", "ptr", "ptr", 8, 70, 300, 44, 10, 10, 0, "null", "null", base, "ptr", "ptr", n_run,
                                 "ptr", "null")],
    "bits sign": lambda n_run, base=BASE: [("sgpt_score_topk_bits", "null", "ptr", "ptr", 8, 70, 300, 44, 10, 40, 1, "null", "null", base, "ptr", "ptr", n_run,
                                 "ptr", "null")],
    "bits fp8": lambda n_run, base=BASE: [("sgpt_score_topk_bits", "null", "ptr", "ptr", 8, 70, 300, 44, 10, 40, 2, "ptr", "ptr", base, "ptr", "ptr", n_run,
                                "ptr", "null")],
    "bits uint8": lambda n_run, base=BASE: [("sgpt_score_topk_bits_u8", "null", "ptr", "null", "ptr", 8, "ptr", "ptr", "ptr", 128, 70, 300, 44, 10, 40, base,
                                  "ptr", "ptr", n_run, "ptr", "null")],
    "bits_centred uint8": lambda n_run, base=BASE: [("sgpt_score_topk_bits_u8", "null", "ptr", "ptr", "ptr", 8, "ptr", "ptr", "ptr", 128, 70, 300, 44, 10, 40,
                                          base, "ptr", "ptr", n_run, "ptr", "null")],
}


@pytest.mark.parametrize("running", [False, True], ids=["fresh", "run"])
@pytest.mark.parametrize("case", sorted(SCORE_CASES))
def test_score_topk_calls(ctx, case, running):
    name, kw = SCORE_CASES[case]
    corpus = _corpora(ctx)[name]
    run = _run() if running else None
    val, idx, n = ctx.score_topk(torch.zeros(NQ, D), corpus, K, idx_base=BASE, run=run, **kw)
    assert ctx.lib.calls == SCORE_EXPECTED[case](3 if running else 0)
    assert val.shape == (NQ, K) and val.dtype == torch.float32 and idx.shape == (NQ, K) and idx.dtype == torch.int64 and n == 0
    if running:
        assert val is run[0] and idx is run[1]


def test_score_topk_refined_calls(ctx):
    """The sixth user of the running list."""
    q, rows = torch.zeros(NQ, 48), torch.zeros(N, 48)
    for run, n_run in ((None, 0), (_run(), 3)):
        ctx.lib.calls.clear()
        val, idx, n = ctx.score_topk_refined(q, rows, rows.to(torch.float16), K, idx_base=BASE, run=run)
        assert ctx.lib.calls == [("sgpt_score_topk_refined", "null", "ptr", "ptr", "ptr", 3, 70, 300, 48, 10, 5, 2.5e-3, "ptr", "ptr", n_run,
                                  "ptr", "null", "null")]
        assert val.shape == (NQ, K) and idx.shape == (NQ, K) and (run is None or (val is run[0] and idx is run[1]))


L2_Q = ("sgpt_l2_normalize", "null", "ptr", NQ, D, "ptr", 0, "null")


@pytest.mark.parametrize("name,case", [("fp8", "fp8"), ("uint8", "uint8"), ("bits", "bits uint8"), ("bits_centred", "bits_centred uint8")])
def test_semantic_search_calls(ctx, name, case):
    """One l2_normalize of the queries, then score_topk's calls with k = top_k, idx_base = 0 and a fresh list; a BinaryCorpus with a
    uint8 copy is re-scored from it."""
    from sgpt_amd import util
    hits = util.semantic_search(torch.zeros(NQ, D), _corpora(ctx)[name], top_k=K)
    assert ctx.lib.calls == [L2_Q] + SCORE_EXPECTED[case](0, base=0)
    assert len(hits) == NQ


def _block_calls(rows, with_fp8, with_u8):
    out = [("sgpt_l2_normalize", "null", "ptr", rows, D, "ptr", 0, "null"),
           ("sgpt_pack_sign_bits", "null", "ptr", rows, D, "null", "ptr", 8, "null")]
    if with_u8:
        out.append(("sgpt_u8_quantize_rows", "null", "ptr", rows, D, 128, "ptr", "ptr", "ptr", "null"))
    if with_fp8:
        out.append(("sgpt_fp8_quantize_rows", "null", "ptr", rows, 48, "ptr", "ptr", "null"))
    return out


def test_binarize_keep_fp8_normalises_each_block_once(ctx):
    """binarize_corpus(keep_fp8=True, block_rows=128) over 300 rows: three blocks (the last ragged), each uploaded and normalised ONCE --
    its sign bits and its fp8 codes come from the same rows.  (Before corpus.py the fp8 copy was a second pass through quantize_corpus:
    three more sgpt_l2_normalize calls.  This is the one record that differs from that commit's.)"""
    corpus = ctx.binarize_corpus(torch.zeros(N, D), keep_fp8=True, block_rows=128)
    assert ctx.lib.calls == [c for rows in (128, 128, 44) for c in _block_calls(rows, True, False)]
    assert sum(c[0] == "sgpt_l2_normalize" for c in ctx.lib.calls) == 3
    assert corpus.bits.shape == (N, 8) and corpus.fp8.codes.shape == (N, 48) and corpus.fp8.scale.shape == (N,) and corpus.fp8.dim == D


def test_builder_calls(ctx):
    """The other builders, block_rows = 128: one upload + normalise + convert per block."""
    emb = torch.zeros(N, D)
    ranges = torch.stack([-torch.ones(D), torch.ones(D)])
    ctx.quantize_corpus(emb, block_rows=128)
    assert ctx.lib.calls == [c for rows in (128, 128, 44) for c in _block_calls(rows, True, False) if c[0] != "sgpt_pack_sign_bits"]
    ctx.lib.calls.clear()
    ctx.quantize_corpus(emb, normalize=False, block_rows=128)
    assert ctx.lib.calls == [("sgpt_fp8_quantize_rows", "null", "ptr", rows, 48, "ptr", "ptr", "null") for rows in (128, 128, 44)]
    ctx.lib.calls.clear()
    ctx.scalar_quantize_corpus(emb, ranges=ranges, block_rows=128)
    assert ctx.lib.calls == [c for rows in (128, 128, 44) for c in _block_calls(rows, False, True) if c[0] != "sgpt_pack_sign_bits"]
    ctx.lib.calls.clear()
    ctx.binarize_corpus(emb, keep_uint8=True, ranges=ranges, block_rows=128)
    assert ctx.lib.calls == [c for rows in (128, 128, 44) for c in _block_calls(rows, False, True)]
