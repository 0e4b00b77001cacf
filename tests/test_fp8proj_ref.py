"""CPU: what the fp8 projections of the Llama family (SGPTModel(projections='fp8'), ABI v25) rest on without a device -- the e4m3fn
tables of the emulation against torch.float8_e4m3fn, the ABI surface, the argument refusals of the Python host, and the emulation's own
deviation from float64 on the test models (tests/fp8proj_ref.py), which profiles/llama_fp8_projections.txt records and the README quotes."""
import os
import re

import numpy as np
import pytest
import torch

import fp8proj_ref as F
from fp8proj_ref import O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "llama_fp8_projections.txt")


# ---- the code tables ------------------------------------------------------------------------------------------------------------

def test_e4m3_tables_agree_with_torch_on_all_256_codes_and_on_ties():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    got = O.fp8_e4m3fn_decode(codes)
    finite = ~np.isnan(want)
    assert finite.sum() == 254 and np.array_equal(got[finite], want[finite])
    # every finite value encodes to its own code (-0 and +0 keep their signs)
    assert np.array_equal(O.fp8_e4m3fn_encode(want[finite]), codes[finite])
    # ties: the midpoint of every pair of neighbouring positive values goes to the even code, in both signs; about 1/16 of bf16 values
    # are such midpoints of the e4m3 grid (4 mantissa bits more, the first one set and the rest clear)
    pos = np.sort(want[finite & (want >= 0)])
    mid = ((pos[:-1].astype(np.float64) + pos[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1].astype(np.float64) + pos[1:]) / 2)        # exact in fp32
    for sign in (1.0, -1.0):
        t = torch.from_numpy(sign * mid).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        mine = O.fp8_e4m3fn_encode(np.float32(sign) * mid)
        assert np.array_equal(mine, t)
        assert (mine & 1 == 0).all()
    # a random sample, bf16 values among it
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(20000) * rng.choice([1e-3, 0.1, 10.0, 300.0], size=20000)).astype(np.float32)
    x = np.concatenate([x, torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()])
    x = x[np.abs(x) <= 448.0]
    assert np.array_equal(O.fp8_e4m3fn_encode(x), torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy())


def test_row_scale_rule():
    amax = np.array([0.0, 448.0, 448.0001, 224.0, 224.0001, 1.75, 1.7500001, 1.0, 3e-39, 1e38], np.float64)
    s = F.pow2_scale(amax)
    assert s[0] == 1.0
    nz = amax[1:] / s[1:]
    assert ((nz <= 448.0) & ((nz > 224.0) | (s[1:] == 2.0 ** -126))).all()
    assert np.array_equal(s[[1, 2, 3, 4, 5, 6, 7]], [1.0, 2.0, 0.5, 1.0, 2.0 ** -8, 2.0 ** -7, 2.0 ** -8])
    assert np.array_equal(O.fp8_scales(amax[:, None].astype(np.float32)).astype(np.float64), F.pow2_scale(amax.astype(np.float32)))
    assert F.switch_margin(1.75) == 0.0 and abs(F.switch_margin(2.0) - 1 / 7) < 1e-12


# ---- the ABI surface --------------------------------------------------------------------------------------------------------------

def test_abi_version_and_new_signatures():
    from sgpt_amd import _lib
    with open(os.path.join(ROOT, "include", "sgpt_hip.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define SGPT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.SGPT_ABI_VERSION >= 25
    for name, nargs in (("sgpt_rmsnorm_fp8", 9), ("sgpt_swiglu_fp8", 8), ("sgpt_model_set_projections", 3), ("sgpt_model_get_projections", 2)):
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"sgpt_status " + name + r"\(([^;]*)\);", hdr)
        assert decl and decl.group(1).count(",") + 1 == nargs, name


# ---- refusals before the device is touched ----------------------------------------------------------------------------------------

class _ContextReached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """SGPTModel(...) that is not refused gets as far as opening the device context, and stops there -- on any machine."""
    import sgpt_amd.model as M

    def stop(device=None):
        raise _ContextReached
    monkeypatch.setattr(M, "get_context", stop)


def refusal(cfg, **kw):
    from sgpt_amd.model import SGPTModel
    with pytest.raises(Exception) as e:
        SGPTModel(cfg, {}, **kw)
    return type(e.value), str(e.value)


def test_projection_refusals(no_device):
    from sgpt_amd.families import SGPTConfig
    ok = F.make_model("llama")[0]
    assert refusal(ok, dtype="bf16", projections="fp8") == (_ContextReached, "")
    assert refusal(ok, dtype="bf16") == (_ContextReached, "")
    assert refusal(ok, dtype="bf16", projections="int8") == (ValueError, "projections must be None or 'fp8', not 'int8'")
    for dtype in ("f16", "fp32"):
        assert refusal(ok, dtype=dtype, projections="fp8") == (ValueError, f"projections='fp8' converts a dtype='bf16' model, not dtype={dtype!r}")
    assert refusal(ok, projections="fp8")[0] is ValueError                              # the default dtype is 'f16'
    kw = dict(vocab_size=100, max_position_embeddings=64, num_layers=1)
    for mt, text in (("gpt_neo", "a GPT-Neo model has dtype 'fp8' / 'fp8mfma'"), ("bloom", "a BLOOM model has dtype 'fp8' / 'fp8mfma'"),
                     ("bert", "a BERT model has no fp8 mode")):
        cfg = SGPTConfig(model_type=mt, hidden_size=256, num_heads=4, **kw)
        assert refusal(cfg, dtype="bf16", projections="fp8") == \
            (ValueError, "projections='fp8' is a mode of the Llama / Mistral / Qwen family: " + text)
    # widths that are not multiples of 256, named
    def llama(**over):
        base = dict(model_type="llama", hidden_size=256, num_heads=4, num_kv_heads=4, intermediate_size=512, window_size=0, **kw)
        base.update(over)
        return SGPTConfig(**base)
    for cfg, name, w in ((llama(hidden_size=384, num_heads=6, num_kv_heads=6), "hidden_size", 384),
                         (llama(hidden_size=256, num_heads=6, rotary_dim=64, num_kv_heads=2), "num_heads * head_dim", 384),
                         (llama(num_kv_heads=2), "num_kv_heads * head_dim", 128),
                         (llama(intermediate_size=640), "intermediate_size", 640)):
        assert refusal(cfg, dtype="bf16", projections="fp8") == \
            (ValueError, f"projections='fp8' needs {name} to be a multiple of 256: this model has {name} = {w}")
        assert refusal(cfg, dtype="bf16") == (_ContextReached, "")


def test_encode_graph_refuses_a_converted_model():
    from sgpt_amd.model import EncodeGraph

    class Stub:
        cfg = F.make_model("llama")[0]
        attention = "causal"
        projections = "fp8"
    with pytest.raises(ValueError, match="EncodeGraph: a model with projections='fp8' is not captured"):
        EncodeGraph(Stub(), [[1, 2, 3]])


def test_from_pretrained_passes_the_keyword_through(monkeypatch, tmp_path):
    import json
    import sgpt_amd.model as M
    seen = {}

    def init(self, cfg, weights, **kw):
        seen.update(kw)
    monkeypatch.setattr(M.SGPTModel, "__init__", init)
    monkeypatch.setattr(M, "load_state_dict", lambda root: {})
    with open(tmp_path / "config.json", "w") as f:
        json.dump(dict(model_type="llama", vocab_size=100, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=512,
                       max_position_embeddings=64, rms_norm_eps=1e-6), f)
    M.SGPTModel.from_pretrained(str(tmp_path), projections="fp8", dtype="bf16")
    assert seen["projections"] == "fp8" and seen["dtype"] == "bf16" and seen["attention"] == "causal"


# ---- the emulation's own deviation from float64 -----------------------------------------------------------------------------------

_E = {}


def emulated_deviation(tag, mode, bidir=False, pool_from=None):
    """(max |de|, max |dcos|) of the emulated unit embeddings against the float64 ones; the forwards are computed once per model."""
    key = (tag, bidir)
    if key not in _E:
        _E[key] = (F.ref_forward(tag, fp8=False, bidir=bidir), F.ref_forward(tag, fp8=True, bidir=bidir))
    ref, emu = _E[key]
    return F.deviation(F.embeddings(emu, mode, pool_from), F.embeddings(ref, mode, pool_from))


def recorded():
    """The E lines of the profile: {(model, mode): max |de|}."""
    with open(PROFILE) as f:
        return {(m.group(1), m.group(2)): float(m.group(3)) for m in re.finditer(r"^E\s+(\w+)\s+(\w+)\s+max\|de\|\s*=\s*(\S+)", f.read(), re.M)}


@pytest.mark.parametrize("tag", list(F.MODELS))
def test_emulated_deviation_from_float64(tag):
    """The deviation is O(1e-2): outside the project's 1e-2 fp8 bar on some models, which is why the mode is opt-in and the README quotes
    these figures.  Asserted: it is finite and below 5e-2 (a wiring error in the emulation is O(1)), above the bf16 forward's own 1e-3
    (the quantisation is live), and the profile records it -- within a factor 1.5, since another BLAS may sum a float64 row in
    another order and one flipped e4m3 code moves a figure by tens of per cent."""
    rec = recorded()
    for mode in F.MODES:
        de, dcos = emulated_deviation(tag, mode)
        print(f"E {tag:6s} {mode:12s} max|de| = {de:.3e}  max|dcos| = {dcos:.3e}")
        assert 1e-3 < de < 5e-2 and dcos < 5e-2, (tag, mode)
        assert (tag, mode) in rec and rec[(tag, mode)] / 1.5 <= de <= rec[(tag, mode)] * 1.5, (tag, mode, de, rec.get((tag, mode)))
