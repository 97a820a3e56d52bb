"""Attention maps on the device (csrc/mha_weights.hip): the one-launch probabilities against an fp64 restatement written
here, against the forward that produced them (weights @ v IS out, dropout mask included), reproducibility, strided and
fully masked inputs, the 16-bit compute dtypes, the module against torch.nn.MultiheadAttention, record_weights on the whole
model, GroundingSession.ground(explain=True) and the refusal under stream capture.

Every bound check prints its measured use of the bound (worst err / tol) before asserting:
`ATTN_WEIGHTS_BOUND <what> <shape> <worst>` -- profiles/attention_weights.md is written from those lines."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# tests/test_attention.py SHAPES: (B, Lq, Lk, masked)
SHAPES = [
    (2, 16, 16, False), (2, 80, 80, True), (1, 1024, 1024, False), (2, 80, 1024, False),
    (2, 1024, 80, True), (2, 1024, 132, True), (2, 256, 256, False), (2, 256, 80, True),
    (3, 37, 101, True), (1, 5, 1, False), (2, 64, 65, True),
    (2, 90, 24, False), (2, 24, 90, True), (2, 110, 175, True),
    (2, 130, 130, True), (2, 130, 1024, False), (2, 1024, 130, True), (2, 256, 130, True),
    (2, 256, 1024, True), (1, 200, 700, True), (8, 80, 1024, True), (8, 256, 1024, False),
]


def _mask(B, L, seed, min_valid=1):
    rng = np.random.default_rng(seed)
    lens = rng.integers(min_valid, L + 1, B)
    lens[0] = L
    return torch.from_numpy(np.arange(L)[None, :] >= lens[:, None])


def _ref_weights(q, k, mask, H=8):
    """fp64: logits per head, -inf on masked keys, softmax -> (B, H, Lq, Lk)."""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    hd = D // H
    qh = q.double().view(B, Lq, H, hd).transpose(1, 2)
    kh = k.double().view(B, Lk, H, hd).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / hd ** 0.5
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    return torch.softmax(s, dim=-1)


def _use_of_bound(got, exp, rel=1e-4):
    """worst |err| / (rel |e| + 2e-6 max|e|): the form and constants of tests/test_attention.py:97 for `out`."""
    err = (got.double() - exp).abs()
    tol = rel * exp.abs() + 2e-6 * exp.abs().max() + 1e-30
    return (err / tol).max().item()


def _heads(v, H=8):
    B, L, D = v.shape
    return v.view(B, L, H, D // H).transpose(1, 2)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("B,Lq,Lk,_m", SHAPES)
def test_weights_kernel_vs_fp64(B, Lq, Lk, _m, masked):
    from eda_amd import attention
    torch.manual_seed(Lq * 7 + Lk)
    dev = "cuda"
    q, k, v = (torch.randn(B, L, 288, device=dev) for L in (Lq, Lk, Lk))
    mask = _mask(B, Lk, Lq + Lk).to(dev) if masked else None
    exp = _ref_weights(q, k, mask)
    plain = attention.attention_core(q, k, v, mask, 8, 0.0, 0)
    for per_head, e in ((True, exp), (False, exp.mean(1))):
        out, w = attention.attention_core_weights(q, k, v, mask, 8, 0.0, 0, per_head=per_head)
        assert torch.equal(out, plain)
        assert w.shape == e.shape and w.dtype == torch.float32 and not w.requires_grad
        worst = _use_of_bound(w, e)
        print(f"ATTN_WEIGHTS_BOUND kernel_{'perhead' if per_head else 'mean'}_{'masked' if masked else 'unmasked'} "
              f"{B}x{Lq}x{Lk} {worst:.3f}")
        assert worst <= 1.0, (per_head, worst)
        if mask is not None:
            dead = mask[:, None, None, :].expand(-1, 8, Lq, -1) if per_head else mask[:, None, :].expand(-1, Lq, -1)
            assert (w[dead] == 0).all()
        assert (w.double().sum(-1) - 1).abs().max().item() <= 1e-4


def _check_weights_make_out(W, v, out, name, shape):
    e = torch.einsum("bhqk,bhkd->bqhd", W.double(), _heads(v).double()).reshape(out.shape)
    worst = _use_of_bound(out, e)
    print(f"ATTN_WEIGHTS_BOUND {name} {shape} {worst:.3f}")
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("B,Lq,Lk", [(2, 256, 1024), (2, 1024, 1024), (2, 256, 80), (3, 37, 101), (2, 1024, 132)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_weights_are_the_ones_the_forward_used(B, Lq, Lk, p):
    """per-head W @ v IS the forward's out -- with dropout only if the keep mask is regenerated identically."""
    from eda_amd import attention
    torch.manual_seed(Lq + 3 * Lk)
    dev = "cuda"
    q, k, v = (torch.randn(B, L, 288, device=dev) for L in (Lq, Lk, Lk))
    mask = _mask(B, Lk, 9, min_valid=max(1, Lk // 2)).to(dev)
    attention.dropout_state(dev).fill_(11)                   # (not bumped between the forward and the weights launch)
    out, W = attention.attention_core_weights(q, k, v, mask, 8, p, 5, per_head=True)
    assert torch.equal(out, attention.attention_core(q, k, v, mask, 8, p, 5))
    _check_weights_make_out(W, v, out, f"W_at_v_is_out_p{p}", f"{B}x{Lq}x{Lk}")
    _, Wm = attention.attention_core_weights(q, k, v, mask, 8, p, 5)
    assert _use_of_bound(Wm, W.double().mean(1)) <= 1.0
    live = ~mask[:, None, None, :].expand(-1, 8, Lq, -1)
    zero_frac = (W[live] == 0).float().mean().item()
    if p == 0.0:
        assert zero_frac == 0.0
    else:
        # test_fused_dropout_statistics_and_gradient_consistency: mean(keep / (1 - p)) within 0.01 of 1
        print(f"ATTN_WEIGHTS_BOUND dropout_zero_fraction {B}x{Lq}x{Lk} {zero_frac:.5f}")
        assert abs((1.0 - zero_frac) / (1.0 - p) - 1.0) < 0.01
        exp = _ref_weights(q, k, mask)
        kept = W != 0
        assert _use_of_bound(torch.where(kept, W * (1.0 - p), W), torch.where(kept, exp, torch.zeros_like(exp))) <= 1.0
        # another call site draws another mask
        _, W2 = attention.attention_core_weights(q, k, v, mask, 8, p, 6, per_head=True)
        assert not torch.equal(W2 == 0, W == 0)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_weights_of_the_fused_q_projection_forward(p):
    """The [q-projection | core] launch (short key sets) leaves q and lse like the two-launch path: the weights launch
    reproduces its probabilities, dropout mask included."""
    from eda_amd import _lib, attention
    torch.manual_seed(4)
    dev = "cuda"
    B, Lq, Lk, d = 4, 256, 80, 288
    assert _lib.lib().eda_mha_qproj_supported(8, 36, Lk)
    x = torch.randn(B, Lq, d, device=dev)
    Wq, bq = torch.randn(d, d, device=dev) / d ** 0.5, torch.randn(d, device=dev) * 0.1
    k, v = torch.randn(B, Lk, d, device=dev), torch.randn(B, Lk, d, device=dev)
    mask = _mask(B, Lk, 3).to(dev)
    m8 = mask.contiguous().view(torch.uint8)
    attention.dropout_state(dev).fill_(23)
    q, out, lse = attention._qproj_core_fwd(x, Wq, bq, k, v, m8, 8, p, 9)
    W = attention._mha_weights_call(q, k, m8, lse, 8, p, 9, True)
    _check_weights_make_out(W, v, out, f"W_at_v_is_out_qproj_p{p}", f"{B}x{Lq}x{Lk}")
    if p == 0.0:
        assert _use_of_bound(W, _ref_weights(q, k, mask)) <= 1.0


def test_module_weights_through_the_fused_q_projection_site(monkeypatch):
    """EDA_MHA_QPROJ=1: the module's cross-attention takes the fused launch; its recorded map is unchanged."""
    from eda_amd import attention
    torch.manual_seed(6)
    mod = attention.MultiheadAttention(288, 8, dropout=0.1).eval().cuda()
    x, mem = torch.randn(2, 256, 288, device="cuda"), torch.randn(2, 80, 288, device="cuda")
    mask = _mask(2, 80, 1).cuda()
    with torch.no_grad():
        o0, w0 = mod(x, mem, mem, key_padding_mask=mask, batch_first=True, need_weights=True)
        monkeypatch.setenv("EDA_MHA_QPROJ", "1")
        o1, w1 = mod(x, mem, mem, key_padding_mask=mask, batch_first=True, need_weights=True)
    assert (o1 - o0).abs().max().item() <= 2e-5 * o0.abs().max().item()
    assert _use_of_bound(w1, w0.double()) <= 1.0


def test_weights_reproducible_strided_and_all_masked():
    from eda_amd import attention
    torch.manual_seed(3)
    dev = "cuda"
    B, L = 2, 200
    packed = torch.randn(B, L, 864, device=dev)
    q, k, v = packed.split(288, dim=-1)
    assert not q.is_contiguous()
    mask = _mask(B, L, 8).to(dev)
    for per_head in (False, True):
        for p in (0.0, 0.1):
            _, a = attention.attention_core_weights(q, k, v, mask, 8, p, 7, per_head=per_head)
            _, b = attention.attention_core_weights(q, k, v, mask, 8, p, 7, per_head=per_head)
            _, c = attention.attention_core_weights(q.contiguous(), k.contiguous(), v.contiguous(), mask, 8, p, 7,
                                                    per_head=per_head)
            assert torch.equal(a, b) and torch.equal(a, c)
    # every key of scene 1 masked: NaN rows, as the forward (test_keys_per_wave_forward_with_all_keys_of_a_scene_masked...)
    q, k, v = (torch.randn(2, n, 288, device=dev) for n in (80, 1024, 1024))
    mask = torch.zeros(2, 1024, dtype=torch.bool, device=dev)
    mask[1] = True
    for per_head in (False, True):
        out, w = attention.attention_core_weights(q, k, v, mask, 8, 0.0, 3, per_head=per_head)
        assert torch.isfinite(w[0]).all() and torch.isnan(w[1]).all()
        assert torch.isfinite(out[0]).all() and torch.isnan(out[1]).all()


def test_entry_point_refuses_other_head_dims():
    from eda_amd import _lib
    L = _lib.lib()
    x = torch.zeros(1, 4, 512, device="cuda")
    lse = torch.zeros(1, 8, 4, device="cuda")
    w = torch.zeros(1, 4, 4, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = L.eda_mha_weights_f32(x.data_ptr(), x.data_ptr(), 2048, 512, 2048, 512, None, lse.data_ptr(), 1, 8, 4, 4, 64,
                               0.125, 0.0, None, 0, 0, w.data_ptr(), st)
    assert rc == 10003                                       # EDA_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="head_dim 36"):
        _lib.check(rc, "eda_mha_weights_f32")
    rc = L.eda_mha_weights_f32(x.data_ptr(), x.data_ptr(), 2048, 512, 2048, 512, None, lse.data_ptr(), 1, 9, 4, 4, 36,
                               0.125, 0.0, None, 0, 0, w.data_ptr(), st)
    assert rc == 10003


@pytest.mark.parametrize("dtype,tol", [("bf16", 2.4e-2), ("f16", 3e-3)])
@pytest.mark.parametrize("B,Lq,Lk,masked", [(2, 80, 1024, False), (2, 256, 132, True)])
def test_weights_with_16bit_compute_dtype(B, Lq, Lk, masked, dtype, tol):
    """The forward's lse comes from the 16-bit contraction, the weights launch stays fp32.  Bound: tol |e| + 2e-6 max|e|
    with the tol tests/test_attention.py:373 places on the same forward against the same restatement.

    Measured on MI355X (worst err / tol): see profiles/attention_weights.md."""
    from eda_amd import attention
    torch.manual_seed(Lq * 5 + Lk)
    dev = "cuda"
    q, k, v = (torch.randn(B, L, 288, device=dev) for L in (Lq, Lk, Lk))
    mask = _mask(B, Lk, Lq + Lk).to(dev) if masked else None
    attention.set_compute_dtype(dtype)
    try:
        _, w = attention.attention_core_weights(q, k, v, mask, 8, 0.0, 0)
        _, wh = attention.attention_core_weights(q, k, v, mask, 8, 0.0, 0, per_head=True)
    finally:
        attention.set_compute_dtype("f32")
    exp = _ref_weights(q, k, mask)
    assert torch.isfinite(w).all() and torch.isfinite(wh).all()
    if mask is not None:
        assert (w[mask[:, None, :].expand(-1, Lq, -1)] == 0).all()
        assert (wh[mask[:, None, None, :].expand(-1, 8, Lq, -1)] == 0).all()
    worst = _use_of_bound(w, exp.mean(1), rel=tol)
    worst_h = _use_of_bound(wh, exp, rel=tol)
    print(f"ATTN_WEIGHTS_BOUND {dtype}_mean {B}x{Lq}x{Lk} {worst:.3f}")
    print(f"ATTN_WEIGHTS_BOUND {dtype}_perhead {B}x{Lq}x{Lk} {worst_h:.3f}")
    assert worst <= 1.0 and worst_h <= 1.0, (worst, worst_h)


@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("batch_first", [True, False])
@pytest.mark.parametrize("case", ["self", "posself", "cross", "distinct"])
def test_module_weights_on_gpu_match_torch_multiheadattention(case, batch_first, average):
    """Bound as in test_module_on_gpu_matches_torch_multiheadattention: 2e-4 x the tensor's scale + 1e-6."""
    from eda_amd import attention
    torch.manual_seed(0)
    ref = torch.nn.MultiheadAttention(288, 8, dropout=0.1).eval().cuda()
    mine = attention.MultiheadAttention(288, 8, dropout=0.1).eval().cuda()
    with torch.no_grad():
        ref.in_proj_bias.normal_(0, 0.1); ref.out_proj.bias.normal_(0, 0.1)
    mine.load_state_dict(ref.state_dict())
    B, Lq, Lk = 4, 256, 80
    x, pos = torch.randn(B, Lq, 288, device="cuda"), torch.randn(B, Lq, 288, device="cuda")
    mem, mem2 = torch.randn(B, Lk, 288, device="cuda"), torch.randn(B, Lk, 288, device="cuda")
    if case == "self":
        q = k = v = x; mask = _mask(B, Lq, 1).cuda()
    elif case == "posself":
        q = k = x + pos; v = x; mask = None
    elif case == "cross":
        q = x + pos; k = v = mem; mask = _mask(B, Lk, 2).cuda()
    else:
        q = x; k = mem; v = mem2; mask = _mask(B, Lk, 3).cuda()
    qt = q.transpose(0, 1)
    kt = qt if k is q else k.transpose(0, 1)
    vt = kt if v is k else (qt if v is q else v.transpose(0, 1))
    with torch.no_grad():
        exp, exp_w = ref(qt, kt, vt, key_padding_mask=mask, need_weights=True, average_attn_weights=average)
        exp = exp.transpose(0, 1)
        if batch_first:
            got, got_w = mine(q, k, v, key_padding_mask=mask, batch_first=True, need_weights=True,
                              average_attn_weights=average)
            plain = mine(q, k, v, key_padding_mask=mask, batch_first=True)
        else:
            got, got_w = mine(qt, kt, vt, key_padding_mask=mask, need_weights=True, average_attn_weights=average)
            plain = mine(qt, kt, vt, key_padding_mask=mask)
            got, plain = got.transpose(0, 1), (plain[0].transpose(0, 1), plain[1])
    assert plain[1] is None and torch.equal(plain[0], got)
    assert got_w.shape == exp_w.shape
    for name, g, e in (("out", got, exp), ("weights", got_w, exp_w)):
        scale = e.abs().max().item() + 1e-9
        assert (g - e).abs().max().item() <= 2e-4 * scale + 1e-6, (name, (g - e).abs().max().item(), scale)
    # the pre-out-projection modes return the same map
    with torch.no_grad():
        o_skip, w_skip = mine(q, k, v, key_padding_mask=mask, batch_first=True, skip_out_proj=True, need_weights=True,
                              average_attn_weights=average)
        o_def, w_def = mine(q, k, v, key_padding_mask=mask, batch_first=True, defer_out_bias=True, need_weights=True,
                            average_attn_weights=average)
        ref_w = mine(q, k, v, key_padding_mask=mask, batch_first=True, need_weights=True, average_attn_weights=average)[1]
    assert torch.equal(w_skip, ref_w) and torch.equal(w_def, ref_w)
    assert o_skip.shape == got.shape and o_def.shape == got.shape


# ---------------------------------------------------------------------------------------------- the whole model
def _site_reference(mod, args, kwargs):
    """fp64 head-mean map of one MultiheadAttention call from its hooked inputs and the module's own in-projection."""
    q_in, k_in = args[0], args[1]
    d = mod.embed_dim
    W, b = mod.in_proj_weight.detach().double(), mod.in_proj_bias.detach().double()
    q = q_in.double() @ W[:d].T + b[:d]
    k = k_in.double() @ W[d:2 * d].T + b[d:2 * d]
    return _ref_weights(q, k, kwargs.get("key_padding_mask"), mod.num_heads).mean(1)


@pytest.mark.parametrize("butd", [True, False])
def test_record_weights_on_the_whole_model(butd):
    import bench
    import check_graph_vs_eager as C
    from eda_amd import attention
    dev = torch.device("cuda", 0)
    model = C.make(0, dev, num_queries=64, num_decoder_layers=2, butd=butd).eval()
    inputs = bench.make_inputs(5, 2, dev, 20000, 24)
    sites = ["cross_encoder.layers.1.self_attention_lang.self_attn", "cross_encoder.layers.1.self_attention_visual.self_attn",
             "cross_encoder.layers.2.cross_layer.cross_lv", "cross_encoder.layers.2.cross_layer.cross_vl",
             "decoder.1.self_attn", "decoder.1.cross_l", "decoder.1.cross_v"]
    if butd:
        sites += ["cross_encoder.layers.0.cross_layer.cross_d", "decoder.1.cross_d"]
    mods = dict(model.named_modules())
    seen = {}
    hooks = [mods[s].register_forward_hook(
        (lambda s_: lambda m, a, kw, out: seen.__setitem__(s_, (a, kw)))(s), with_kwargs=True) for s in sites]
    with torch.no_grad():
        base = model(inputs)
        with attention.record_weights(model, sites) as maps:
            rec = model(inputs)
        after = model(inputs)
    for h in hooks:
        h.remove()
    assert set(maps) == set(sites)
    n_maps = {s: maps[s].clone() for s in sites}
    for name, t in base.items():
        if torch.is_tensor(t):
            assert torch.equal(t, rec[name]), name
            assert torch.equal(t, after[name]), name
    assert all(torch.equal(maps[s], n_maps[s]) for s in sites)          # nothing recorded after the context
    am = inputs["tokenized"]["attention_mask"]
    for s in sites:
        a, kw = seen[s]
        exp = _site_reference(mods[s], a, kw)
        assert maps[s].shape == exp.shape, s
        worst = _use_of_bound(maps[s], exp)
        print(f"ATTN_WEIGHTS_BOUND model_{'butd' if butd else 'nobutd'}_{s} {tuple(exp.shape)} {worst:.3f}")
        assert worst <= 1.0, (s, worst)
    pad = (am == 0)[:, None, :].expand(-1, maps["decoder.1.cross_l"].shape[1], -1)
    assert pad.any() and (maps["decoder.1.cross_l"][pad] == 0).all()
    with pytest.raises(KeyError, match="decoder.1.cross_l"):
        attention.record_weights(model, ["decoder.9.cross_l"])
    with pytest.raises(KeyError, match="ambiguous"):
        attention.record_weights(model, ["cross_l"])


def test_ground_explain():
    import bench
    import check_graph_vs_eager as C
    from eda_amd import attention
    from eda_amd.inference import GroundingSession, upsample_to_points
    dev = torch.device("cuda", 0)
    U, points, tokens = 5, 20000, 24
    model = C.make(0, dev, num_queries=64, num_decoder_layers=2).eval()
    inputs = bench.make_inputs(3, U, dev, points, tokens)
    scene = inputs["point_clouds"][0]
    tok = inputs["tokenized"]
    det = (inputs["det_boxes"][0], inputs["det_bbox_label_mask"][0], inputs["det_class_ids"][0])
    calls = []
    inner = model.forward_point_backbone
    model.forward_point_backbone = lambda x: (calls.append(1), inner(x))[1]
    session = GroundingSession(model)
    with torch.no_grad():
        plain = session.ground(scene, tok, detected_boxes=det, topk=10)
        assert "explain" not in plain and len(calls) == 1
        with attention.record_weights(model, ["decoder.1.cross_l", "decoder.1.cross_v"]) as full:
            res = session.ground(scene, tok, detected_boxes=det, topk=10, explain=True)
        assert len(calls) == 2                               # the point backbone still runs once per call
        reuse = session.ground(None, tok, detected_boxes=det, topk=10, explain=True, scene=res["scene"])
        assert len(calls) == 2
    torch.cuda.synchronize()
    for k in ("boxes", "scores", "queries", "corners"):
        assert torch.equal(res[k], plain[k]), k
        assert torch.equal(reuse[k], plain[k]), k
    ex = res["explain"]
    S, L = 1024, tok["input_ids"].shape[1]
    assert ex["token_to_seeds"].shape == (U, L, S)
    assert ex["query_to_tokens"].shape == (U, 10, L) and ex["query_to_seeds"].shape == (U, 10, S)
    assert ex["seed_xyz"].shape == (S, 3) and ex["seed_inds"].shape == (S,)
    assert torch.equal(ex["seed_xyz"], scene[ex["seed_inds"].long(), :3])
    qi = res["queries"].long()
    for u in range(U):
        assert torch.equal(ex["query_to_tokens"][u], full["decoder.1.cross_l"][u, qi[u]])
        assert torch.equal(ex["query_to_seeds"][u], full["decoder.1.cross_v"][u, qi[u]])
    assert (ex["token_to_seeds"].sum(-1) - 1).abs().max().item() <= 1e-4
    assert (ex["query_to_tokens"][(tok["attention_mask"] == 0)[:, None, :].expand(-1, 10, -1)] == 0).all()
    for k in ex:
        assert torch.equal(ex[k], reuse["explain"][k]), k
    # colouring the cloud
    for seed_map in (ex["query_to_seeds"], ex["query_to_seeds"][0, 0], ex["token_to_seeds"][1]):
        up = upsample_to_points(seed_map, res["scene"])
        assert up.shape == (*seed_map.shape[:-1], points)
        lo, hi = seed_map.min(-1, keepdim=True)[0], seed_map.max(-1, keepdim=True)[0]
        eps = 1e-6 * hi
        assert bool(((up >= lo - eps) & (up <= hi + eps)).all())
        at_seeds = up[..., ex["seed_inds"].long()]
        assert (at_seeds - seed_map).abs().max().item() <= 1e-4 * seed_map.max().item()


def test_record_weights_refuses_stream_capture():
    from eda_amd import attention
    torch.manual_seed(0)
    mod = torch.nn.ModuleDict({"attn": attention.MultiheadAttention(288, 8).eval().cuda()})
    x = torch.randn(2, 64, 288, device="cuda")
    with torch.no_grad():
        mod["attn"](x, x, x, batch_first=True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with attention.record_weights(mod, ["attn"]) as maps:
            with pytest.raises(RuntimeError, match="captured"):
                with torch.cuda.graph(g):
                    y = x + 1.0
                    mod["attn"](y, y, y, batch_first=True)
            assert not maps
            torch.cuda.synchronize()
            mod["attn"](x, x, x, batch_first=True)            # eager: recorded
        assert maps["attn"].shape == (2, 64, 64)
