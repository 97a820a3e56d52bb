"""Attention maps on the CPU path: MultiheadAttention(need_weights=True) against torch.nn.MultiheadAttention, the untouched
default path, and the record_weights context manager.  (The HIP launch is tested in test_attention_weights_gpu.py against
the same torch form.)"""
import numpy as np
import pytest
import torch

from oracle import attention_ref


def _mask(B, L, seed, min_valid=1):
    rng = np.random.default_rng(seed)
    lens = rng.integers(min_valid, L + 1, B)
    lens[0] = L
    return torch.from_numpy(np.arange(L)[None, :] >= lens[:, None])


def _pair():
    from eda_amd import attention
    torch.manual_seed(0)
    ref = torch.nn.MultiheadAttention(288, 8, dropout=0.1).eval()
    mine = attention.MultiheadAttention(288, 8, dropout=0.1).eval()
    with torch.no_grad():
        ref.in_proj_bias.normal_(0, 0.1); ref.out_proj.bias.normal_(0, 0.1)
    mine.load_state_dict(ref.state_dict())
    return ref, mine


def _inputs(case, masked):
    B, Lq, Lk = 3, 20, 33
    x = torch.randn(B, Lq, 288); pos = torch.randn(B, Lq, 288); mem = torch.randn(B, Lk, 288)
    if case == "self":
        return x, x, x, (_mask(B, Lq, 1) if masked else None)
    if case == "posself":
        return x + pos, None, x, (_mask(B, Lq, 3) if masked else None)       # (None: key IS query)
    return x, mem, mem, (_mask(B, Lk, 2) if masked else None)


@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("batch_first", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("case", ["self", "posself", "cross"])
def test_module_weights_match_torch_multiheadattention(case, masked, batch_first, average, monkeypatch):
    from eda_amd import attention
    monkeypatch.setattr(attention, "_core", attention_ref.attention_core)
    ref, mine = _pair()
    q, k, v, mask = _inputs(case, masked)
    k = q if k is None else k
    qt = q.transpose(0, 1)
    kt = qt if k is q else k.transpose(0, 1)
    vt = kt if v is k else (qt if v is q else v.transpose(0, 1))
    exp, exp_w = ref(qt, kt, vt, key_padding_mask=mask, need_weights=True, average_attn_weights=average)
    exp = exp.transpose(0, 1)
    if batch_first:
        got, got_w = mine(q, k, v, key_padding_mask=mask, batch_first=True, need_weights=True, average_attn_weights=average)
        plain = mine(q, k, v, key_padding_mask=mask, batch_first=True)
    else:
        got, got_w = mine(qt, kt, vt, key_padding_mask=mask, need_weights=True, average_attn_weights=average)
        plain = mine(qt, kt, vt, key_padding_mask=mask)
        got, plain = got.transpose(0, 1), (plain[0].transpose(0, 1), plain[1])
    assert got_w is not None and got_w.shape == exp_w.shape == ((3, 20, k.shape[1]) if average else (3, 8, 20, k.shape[1]))
    torch.testing.assert_close(got_w, exp_w, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got, exp, rtol=1e-5, atol=1e-5)
    assert not got_w.requires_grad
    # the default path: second element None, same output bits
    assert plain[1] is None and torch.equal(plain[0], got)
    if mask is not None:
        dead = mask[:, None, :].expand(-1, 20, -1) if average else mask[:, None, None, :].expand(-1, 8, 20, -1)
        assert (got_w[dead] == 0).all()


def test_defer_out_bias_and_attn_mask(monkeypatch):
    from eda_amd import attention
    monkeypatch.setattr(attention, "_core", attention_ref.attention_core)
    _, mine = _pair()
    x = torch.randn(2, 9, 288)
    o, b = mine(x, x, x, batch_first=True, defer_out_bias=True)
    assert b is mine.out_proj.bias
    o2, w = mine(x, x, x, batch_first=True, defer_out_bias=True, need_weights=True)
    assert torch.equal(o, o2) and w.shape == (2, 9, 9)
    torch.testing.assert_close(w.sum(-1), torch.ones(2, 9), rtol=0, atol=1e-5)
    with pytest.raises(NotImplementedError):
        mine(x, x, x, attn_mask=torch.zeros(9, 9), need_weights=True)


def test_attention_core_weights_cpu_form():
    from eda_amd import attention
    torch.manual_seed(1)
    q, k, v = torch.randn(2, 7, 288, requires_grad=True), torch.randn(2, 11, 288), torch.randn(2, 11, 288)
    mask = _mask(2, 11, 4)
    out, w = attention.attention_core_weights(q, k, v, mask, 8, 0.0, 0, per_head=True)
    assert w.shape == (2, 8, 7, 11) and not w.requires_grad and out.requires_grad
    exp = attention_ref.attention_core(q.detach().double(), k.double(), v.double(), mask, 8)
    torch.testing.assert_close(out.detach().double(), exp, rtol=1e-5, atol=1e-5)
    vh = v.view(2, 11, 8, 36).transpose(1, 2)
    torch.testing.assert_close((w @ vh).transpose(1, 2).reshape(2, 7, 288), out.detach(), rtol=1e-5, atol=1e-5)
    _, wa = attention.attention_core_weights(q, k, v, mask, 8, 0.0, 0)
    torch.testing.assert_close(wa, w.mean(1), rtol=1e-6, atol=1e-7)
    assert (wa[mask[:, None, :].expand(-1, 7, -1)] == 0).all()


def test_record_weights_on_a_decoder_layer(monkeypatch):
    from eda_amd import attention
    from eda_amd.encoder_decoder_layers import BiDecoderLayer
    monkeypatch.setattr(attention, "_core", attention_ref.attention_core)
    torch.manual_seed(2)
    layer = BiDecoderLayer(288, n_heads=8, dim_feedforward=256, dropout=0.1, self_position_embedding="none",
                           butd=True).eval()
    names = [n for n, m in layer.named_modules() if isinstance(m, attention.MultiheadAttention)]
    assert set(names) == {"self_attn", "cross_l", "cross_d", "cross_v"}
    B, Q, L, D, S = 2, 12, 9, 7, 40
    query, vis, text, det = (torch.randn(B, n, 288) for n in (Q, S, L, D))
    tmask, dmask = _mask(B, L, 5), _mask(B, D, 6)

    def run():
        with torch.no_grad():
            return layer(query, vis, text, None, None, tmask, detected_feats=det, detected_mask=dmask)
    base = run()
    with attention.record_weights(layer, ["self_attn", "cross_l", "cross_v"]) as maps:
        out = run()
        assert set(maps) == {"self_attn", "cross_l", "cross_v"}
        for name, lk in (("self_attn", Q), ("cross_l", L), ("cross_v", S)):
            assert maps[name].shape == (B, Q, lk), name
            assert (maps[name].sum(-1) - 1).abs().max().item() <= 1e-5, name
        assert (maps["cross_l"][tmask[:, None, :].expand(-1, Q, -1)] == 0).all()
    assert torch.equal(out, base)
    with attention.record_weights(layer, "cross_d", per_head=True) as maps:
        run()
    assert maps["cross_d"].shape == (B, 8, Q, D)
    assert (maps["cross_d"].sum(-1) - 1).abs().max().item() <= 1e-5
    # after the context: nothing is recorded, nothing changes
    n_before = {k: v.clone() for k, v in maps.items()}
    assert attention._recording is None
    assert torch.equal(run(), base)
    assert set(maps) == set(n_before) and all(torch.equal(maps[k], n_before[k]) for k in maps)
    with pytest.raises(KeyError, match="cross_l"):
        attention.record_weights(layer, ["cross_x"])
    with pytest.raises(KeyError, match="ambiguous"):
        attention.record_weights(torch.nn.ModuleList([layer, BiDecoderLayer(288, n_heads=8, dim_feedforward=256)]), ["cross_l"])
    with attention.record_weights(torch.nn.ModuleList([layer]), ["0.cross_l"]) as maps:       # a unique suffix / full name
        run()
    assert maps["0.cross_l"].shape == (B, Q, L)


def test_record_weights_contexts_nest(monkeypatch):
    """An inner context on the same module (GroundingSession.ground(explain=True) inside a caller's own) does not take
    the outer one's map away; per-head and head-mean recorders are served from one computation."""
    from eda_amd import attention
    monkeypatch.setattr(attention, "_core", attention_ref.attention_core)
    torch.manual_seed(3)
    mod = torch.nn.ModuleDict({"a": attention.MultiheadAttention(288, 8).eval(), "b": attention.MultiheadAttention(288, 8).eval()})
    x = torch.randn(2, 6, 288)
    with torch.no_grad():
        with attention.record_weights(mod, ["a", "b"]) as outer:
            with attention.record_weights(mod, ["a"], per_head=True) as inner:
                mod["a"](x, x, x, batch_first=True)
                mod["b"](x, x, x, batch_first=True)
            assert set(inner) == {"a"} and inner["a"].shape == (2, 8, 6, 6)
            assert set(outer) == {"a", "b"} and outer["a"].shape == (2, 6, 6)
            torch.testing.assert_close(outer["a"], inner["a"].mean(1), rtol=1e-6, atol=1e-7)
            before = inner["a"].clone()
            mod["a"](2 * x, x, x, batch_first=True)             # the inner context is closed: only the outer one records
            assert torch.equal(inner["a"], before) and not torch.equal(outer["a"], before.mean(1))
    assert attention._recording is None
