"""CPU: the float64 attention reference of the GPU attention tests (tests/attn_ref.py) against a second, independent
implementation -- torch.nn.functional.scaled_dot_product_attention in float64, given an explicit boolean mask (and, for
ALiBi, an additive bias built from it) -- over random packed layouts with windows, odd lengths and sharp logits."""
import numpy as np
import pytest
import torch

from attn_ref import layout, packed_attention, visible
from oracle import sgpt_oracle as O


def _sdpa(q, k, v, off, lens, H, window, scale, slopes):
    rows, d = q.shape
    dh = d // H
    out = np.full((rows, d), np.nan)
    for s0, n in zip(off.tolist(), lens.tolist()):
        qs, ks, vs = (torch.from_numpy(a[s0:s0 + n]).reshape(n, H, dh).transpose(0, 1) for a in (q, k, v))
        mask = torch.from_numpy(visible(n, window))
        if slopes is None:
            m = mask
        else:
            bias = torch.from_numpy(np.asarray(slopes, np.float64))[:, None, None] * torch.arange(n, dtype=torch.float64)[None, None, :]
            m = torch.where(mask[None], bias.expand(H, n, n), torch.tensor(-np.inf, dtype=torch.float64))
        o = torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, attn_mask=m, scale=scale)
        out[s0:s0 + n] = o.transpose(0, 1).reshape(n, d).numpy()
    return out


@pytest.mark.parametrize("seed", range(6))
def test_reference_matches_torch_sdpa_float64(seed):
    rng = np.random.default_rng(seed)
    H, dh = int(rng.choice([2, 3, 4])), int(rng.choice([8, 16]))
    lens = rng.integers(1, 90, size=int(rng.integers(1, 6)))
    lens[0] = int(rng.choice([1, 2, 65, 129]))                     # odd lengths and tile edges
    window = int(rng.choice([0, 1, 8, 40, 64]))
    scale = float(rng.choice([1.0, dh ** -0.5]))
    slopes = O.alibi_slopes(H) if seed % 2 else None
    off, alloc, T, _ = layout(lens)
    q, k, v = (rng.standard_normal((T, H * dh)) * 2.0 for _ in range(3))
    # sharp logits: a few keys 10 above the rest for their query (the regime the GPU tests run in)
    for s0, n in zip(off.tolist(), lens.tolist()):
        for i in rng.integers(0, n, size=min(n, 4)).tolist():
            j = int(rng.integers(0, i + 1))
            q[s0 + i, :dh] = 0.0
            q[s0 + i, 0] = 1.0
            k[s0 + j, :dh] = 0.0
            k[s0 + j, 0] = 10.0 / scale
    want = _sdpa(q, k, v, off, lens, H, window, scale, slopes)
    got = packed_attention(q, k, v, off, lens, H, window, scale, slopes)
    real = np.zeros(T, bool)
    for s0, n in zip(off.tolist(), lens.tolist()):
        real[s0:s0 + n] = True
    assert np.isnan(got[~real]).all()
    assert np.abs(got[real] - want[real]).max() < 1e-12 * np.abs(v).max()


def test_reference_window_rule_and_alibi_positions():
    """Hand-checkable: one-hot values pick out which keys carry weight."""
    n, H, dh = 6, 1, 4
    off, _, T, _ = layout([n])
    q = np.zeros((T, dh))
    k = np.zeros((T, dh))
    v = np.zeros((T, dh))
    v[:n, 0] = np.arange(n)                                        # context column 0 = the expected key index
    out = packed_attention(q, k, v, off, [n], H, window=2)         # equal scores: uniform over keys {i-1, i}
    assert np.allclose(out[:n, 0], [0.0, 0.5, 1.5, 2.5, 3.5, 4.5])
    out = packed_attention(q, k, v, off, [n], H, window=0, slopes=[50.0])   # steep ALiBi: the latest visible key wins
    assert np.allclose(out[:n, 0], np.arange(n), atol=1e-12)
