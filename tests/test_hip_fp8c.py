"""projection_mode "fp16-fp8c" (DIGAT_GEMM_F16F8C, BASELINE configs[4] on the fp8 matrix cores): the Eq. 8 node projections as
x_hi w_hi on the fp16 matrix cores plus the two corrections q(x_hi) q(w_lo) + q(x_lo) q(w_hi) on the block-scaled
v_mfma_scale_f32_16x16x128_f8f6f4 (OCP e4m3, one E8M0 scale per 32 K values).  CPU tests: the ABI, the size function, the flag
bits and the command-line switch.  GPU tests: the product against a torch restatement of the quantiser and against fp64, one
Eq. 8 layer against the oracle, the refusal of mismatched images, and the trained reference-pinned dev set at the reference's
own 1e-4."""
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------- CPU
def test_library_exports_the_f16f8c_symbols():
    from digat_amd import _lib
    assert "digat_split_weights_bytes_format" in _lib.EXPORTED
    assert _lib.GEMM_F16F8C == 2 and _lib.PARAMS_PROJ_F16F8C == 4096
    L = _lib.lib()
    assert hasattr(L, "digat_split_weights_bytes_format")
    header = open(os.path.join(ROOT, "include", "digat_hip.h")).read()
    assert "DIGAT_GEMM_F16F8C = 2" in header and "DIGAT_PARAMS_PROJ_F16F8C = 4096" in header


@pytest.mark.parametrize("d", [64, 400, 800])
def test_split_size_covers_the_f16f8c_image(d):
    """Per (80-row strip, 128-deep K tile): 20 480 bytes of fp16 w_hi, 2 x 10 240 of e4m3 codes, 1 024 of scale bytes."""
    from digat_amd import _lib
    L = _lib.lib()
    rows = 3 * d
    image = ((rows + 79) // 80) * ((d + 127) // 128) * (80 * 128 * 2 + 2 * 80 * 128 + 1024)
    assert L.digat_split_weights_bytes_format(rows, d, _lib.GEMM_F16F8C) >= image
    # the old size function is unchanged, and formats 0 / 1 give exactly it
    old = ((rows + 79) // 80) * ((d + 31) // 32) * 960 * 16
    assert L.digat_split_weights_bytes(rows, d) == old
    for f in (_lib.GEMM_BF16X6, _lib.GEMM_F16X3):
        assert L.digat_split_weights_bytes_format(rows, d, f) == old
    assert L.digat_split_weights_bytes_format(rows, d, 7) == 0


def _encoder(d=400, L=2):
    from digat_amd.graphEncoders import DIGAT
    cfg = types.SimpleNamespace(news_graph_size=10, max_history_num=50, category_num=17, graph_depth=L, dropout_rate=0.2)
    return DIGAT(cfg, d)


def test_fp16_fp8c_mode_sets_the_documented_flags():
    from digat_amd import _lib
    enc = _encoder().eval()
    enc.projection_mode = "fp16-fp8c"
    assert enc.resolved_projection_mode() == "fp16-fp8c"
    assert enc.gemm_format() == _lib.GEMM_F16X3              # every other image of the block stays fp16x3 (bit 6)
    flags = enc._flags()
    assert flags & _lib.PARAMS_PROJ_F16F8C and flags & _lib.PARAMS_GEMM_F16X3
    assert not flags & (4 | 16 | 32 | 256)                   # no PQ_X3 / PQ_BF16 / PQ_X1 / PQ_FP8 with it
    key = enc._fold_key()
    enc.projection_mode = "fp16x3"
    assert not enc._flags() & _lib.PARAMS_PROJ_F16F8C and enc._fold_key() != key
    for mode in ("auto", "bf16x6", "pq-bf16", "pq-fp8"):
        enc.projection_mode = mode
        assert not enc._flags() & _lib.PARAMS_PROJ_F16F8C


def test_config_parses_inference_projection():
    from digat_amd.config import Config
    assert Config([]).inference_projection == "auto"
    assert Config(["--inference_projection", "fp16-fp8c"]).inference_projection == "fp16-fp8c"
    with pytest.raises(SystemExit):
        Config(["--inference_projection", "fp7"])


# ----------------------------------------------------------------------------------------------------------- GPU
def _fp16_rtz(v):
    """fp32 -> the fp16 value nearest zero (v_cvt_pkrtz_f16_f32), |v| < 65504: drop the mantissa bits fp16 does not hold."""
    bits = v.view(torch.int32)
    normal = (bits & 0x7FFFFFFF) >= 0x38800000                 # |v| >= 2^-14: 10 mantissa bits
    trunc = (bits & ~0x1FFF).view(torch.float32)
    sub = torch.trunc(v * 2.0 ** 24) * 2.0 ** -24               # subnormal fp16: quantum 2^-24
    return torch.where(normal, trunc, sub)


def _mx_e4m3(v):
    """[..., K] (K % 32 == 0) -> OCP e4m3 with one E8M0 scale per 32 values: the least 2^e with absmax / 2^e <= 448, codes
    rounded to nearest even; returned dequantised (fp32 values)."""
    shp = v.shape
    vb = v.reshape(*shp[:-1], shp[-1] // 32, 32)
    amax = vb.abs().amax(-1, keepdim=True)
    u = amax.view(torch.int32)
    x = (u >> 23) - 8 + ((u & 0x7FFFFF) > 0x600000).to(torch.int32)
    x = x.clamp(0, 253)
    inv = ((254 - x) << 23).view(torch.float32)               # 2^(127 - x)
    scale = torch.pow(2.0, (x - 127).to(torch.float64))        # 2^(x - 127)
    q = (vb * inv).to(torch.float8_e4m3fn).to(torch.float64) * scale
    return q.reshape(shp)


def emulate_f16f8c(x, w, b):
    """The product DIGAT_GEMM_F16F8C computes, restated in torch with fp64 sums: activations x 2^4 and weights x 2^10 (exact),
    x_hi = fp16 truncation, w_hi = fp16 rounding, the remainders exact in fp32; result = x_hi w_hi + q(x_hi) q(w_lo) +
    q(x_lo) q(w_hi), scaled back, + bias."""
    M, K = x.shape
    Kp = -(-K // 128) * 128
    xp = torch.zeros(M, Kp, dtype=torch.float32)
    wp = torch.zeros(w.shape[0], Kp, dtype=torch.float32)
    xp[:, :K] = x
    wp[:, :K] = w
    xs = xp * 16.0
    xh = _fp16_rtz(xs)
    xl = xs - xh
    ws = wp * 1024.0
    wh = ws.to(torch.float16).to(torch.float32)
    wl = ws - wh
    y = (xh.double() @ wh.double().T + _mx_e4m3(xh) @ _mx_e4m3(wl).T + _mx_e4m3(xl) @ _mx_e4m3(wh).T) / (1024.0 * 16.0)
    return y + b.double()


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(4100, 1200, 400), (37, 240, 400), (4100, 400, 416)])
def test_f16f8c_linear_against_its_quantiser_and_fp64(M, N, K):
    """digat_linear_f32x3(..., DIGAT_GEMM_F16F8C) at any M (37 rows: no fall-back to another kernel — none reads this image).

    (1) Against the torch restatement of the exact quantiser: the kernel's only freedom is the fp32 accumulation order, so the
    difference is at most 1e-6 of the row's largest |y|.
    (2) Against fp64 x @ w.T.  Bound, derived: the leading product x_hi w_hi is exact in the fp32 accumulator's terms; the
    dropped x_lo w_lo is <= 2^-10 2^-11 |x w| per term.  Each correction operand is an e4m3 code with a relative step of at most
    2^-3, so round-to-nearest errs by <= 2^-4 per operand and a correction product by <= (2 2^-4 + 2^-8) of itself; the
    corrections are <= 2^-11 |x w| (w_lo: half an fp16 ulp of w_hi) and < 2^-10 |x w| (x_lo: a truncation remainder), so a term
    errs by < 2^-3.9 (2^-11 + 2^-10) |x w| < 2^-12 |x_k w_k| — summed: |err| <= 2^-12 sum_k |x_k w_k| (+ 1e-6 of the row for the
    fp32 accumulation), the worst case.  Typical: the errors are rounding noise of rms ~2^-4.8 on corrections of rms ~2^-11 of
    each term, i.e. ~2^-15.8 per term, so rms(err / sqrt(sum_k (x_k w_k)^2)) <= 2^-14 (measured below; the scheme's 2^-15)."""
    from digat_amd import _lib
    rng = np.random.default_rng(M + N + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    xt, wt, bt = (torch.from_numpy(a) for a in (x, w, b))
    L = _lib.lib()
    xd, wd, bd = (t.to(DEV) for t in (xt, wt, bt))
    y = torch.full((M, N), float("nan"), device=DEV)
    ws = torch.empty(L.digat_split_weights_bytes_format(N, K, _lib.GEMM_F16F8C), dtype=torch.uint8, device=DEV)
    _lib.check(L.digat_linear_f32x3(xd.data_ptr(), K, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), N, M, N, K, ws.data_ptr(),
                                    _lib.GEMM_F16F8C, _lib.stream_ptr()), "digat_linear_f32x3 f16f8c")
    torch.cuda.synchronize()
    got = y.cpu().double()
    assert torch.isfinite(got).all()
    emu = emulate_f16f8c(xt, wt, bt)
    row = emu.abs().amax(1, keepdim=True)
    e_emu = ((got - emu).abs() / row).max().item()
    exact = xt.double() @ wt.double().T + bt.double()
    err = (got - exact).abs()
    l1 = xt.double().abs() @ wt.double().abs().T
    l2 = (xt.double() ** 2) @ (wt.double() ** 2).T
    worst = (err / (2.0 ** -12 * l1 + 1e-6 * exact.abs().amax(1, keepdim=True))).max().item()
    rms = torch.sqrt(((err / l2.sqrt()) ** 2).mean()).item()
    print(f"\n[f16f8c {M}x{N}x{K}] vs quantiser: max {e_emu:.2e} of the row; vs fp64: worst-case ratio {worst:.3f}, "
          f"rms err / sqrt(sum (x w)^2) {rms:.2e} (2^-15 = {2.0 ** -15:.2e})")
    assert e_emu <= 1e-6
    assert worst <= 1.0
    assert rms <= 2.0 ** -14
    # the corrections ran: without them (x_hi w_hi alone) the error is ~2^-11, far above what is measured
    assert rms < 2.0 ** -13


@pytest.mark.gpu
def test_f16f8c_eq8_layer_against_the_oracle_and_image_refusal():
    """digat_xattn_fwd_lowprec(format = DIGAT_GEMM_F16F8C, pq = 0): one Eq. 8 layer of MIND-shaped user graphs (B n = 3 216 node
    rows) against the oracle's cross_graph_attention.  And the format registry: an fp16x3 image named as F16F8C, and the
    reverse, return DIGAT_ERR_ARG (1); pq != 0 with F16F8C too."""
    from digat_amd import _lib, synthetic
    from oracle import digat_oracle as O
    B, N, H, C, d, L = 48, 10, 50, 17, 400, 1
    state = synthetic.make_state_dict(d, C, L, seed=181, bias_std=0.05)
    batch = synthetic.make_encoder_batch(B, N, H, C, d, seed=182, empty_history_rows=(2,))
    p = O.as_params(state)
    tb = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()}
    pre = "user_graph_attention_"
    with torch.no_grad():
        Xu = O.user_nodes(p, tb["user_news_embedding"])
        c_n = O.news_graph_context(p, tb["news_graph_embeddings"], tb["news_graph_mask"])
        want = O.cross_graph_attention(p, "user", 0, Xu, tb["user_graph"], c_n)
    U = Xu.shape[1]
    assert B * U >= 2048
    Lb = _lib.lib()
    dev = torch.device(DEV)
    w = {k: torch.from_numpy(state[f"{pre}{k}"]).to(dev).contiguous() for k in
         ("W.0.weight", "W.0.bias", "ffn1.0.weight", "ffn2.0.weight", "ffn3.0.weight", "ffn3.0.bias", "a.0.weight")}

    def split(fmt):
        img = torch.empty(Lb.digat_split_weights_bytes_format(3 * d, d, fmt), dtype=torch.uint8, device=dev)
        _lib.check(Lb.digat_split_proj_weights(w["W.0.weight"].data_ptr(), w["ffn1.0.weight"].data_ptr(), w["ffn2.0.weight"].data_ptr(),
                                               d, img.data_ptr(), fmt, _lib.stream_ptr()), "split")
        return img
    img8, img16 = split(_lib.GEMM_F16F8C), split(_lib.GEMM_F16X3)
    dX, dA, dc = Xu.to(dev).contiguous(), tb["user_graph"].to(dev).contiguous(), c_n.to(dev).contiguous()
    out = torch.full((B, U, d), float("nan"), device=dev)
    nbytes = Lb.digat_xattn_workspace_bytes(B, U, d)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)

    def layer(img, fmt, pq=0):
        return Lb.digat_xattn_fwd_lowprec(dX.data_ptr(), dA.data_ptr(), dc.data_ptr(), w["W.0.weight"].data_ptr(), w["W.0.bias"].data_ptr(),
                                          w["ffn1.0.weight"].data_ptr(), w["ffn2.0.weight"].data_ptr(), w["ffn3.0.weight"].data_ptr(),
                                          w["ffn3.0.bias"].data_ptr(), w["a.0.weight"].data_ptr(), img.data_ptr(), fmt, out.data_ptr(),
                                          B, U, d, pq, ws.data_ptr(), nbytes, _lib.stream_ptr())
    assert layer(img16, _lib.GEMM_F16F8C) == 1, "an fp16x3 image named as F16F8C must be refused"
    assert layer(img8, _lib.GEMM_F16X3) == 1, "an F16F8C image named as fp16x3 must be refused"
    assert layer(img8, _lib.GEMM_F16F8C, pq=1) == 1
    _lib.check(layer(img8, _lib.GEMM_F16F8C), "digat_xattn_fwd_lowprec f16f8c")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    scale = float(want.abs().max())
    print(f"\n[Eq. 8 layer, F16F8C] vs the oracle: max {err.max():.3e} mean {err.mean():.3e} (output scale {scale:.2f})")
    assert err.max() <= 1e-4 * scale


def _trained():
    from conftest import planted_devset
    from digat_amd import util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    fx, corpus, state = planted_devset()
    spec = corpus.spec
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=int(fx["depth"]),
                                dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model = model.to(DEV).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, torch.device(DEV))
    return fx, corpus, model, dc


@pytest.mark.gpu
def test_trained_model_fp16_fp8c_holds_the_reference_tolerance():
    """The acceptance test: the trained, reference-pinned dev set (tests/golden/devset_trained_2k.npz; AUC ~0.64, logits of rms
    ~10) scored with projection_mode "fp16-fp8c": AUC / MRR / nDCG@5 / nDCG@10 within the reference's own 1e-4, scores within
    2e-5 of the largest |score|, >= 99.9 % of the ranks equal.  Live-row lists on and off give the same bits (the row-list
    launches of the projection GEMM compute the same rows as the contiguous ones)."""
    from digat_amd import evaluate, util
    fx, corpus, model, dc = _trained()
    enc = model.graph_encoder
    enc.projection_mode = "fp16x3"
    base, _ = util.compute_scores(model, dc, 1024, labels=corpus.row_label)
    enc.projection_mode = "fp16-fp8c"
    scores, metrics = util.compute_scores(model, dc, 1024, labels=corpus.row_label)
    assert not np.array_equal(scores, base), "the fp16-fp8c path did not run"
    ref = fx["scores"].astype(np.float64)
    err = np.abs(scores - ref)
    drift = np.abs(np.array(metrics) - fx["metrics"])
    ranks = np.asarray(evaluate.impression_ranks(scores, corpus.row_impression))
    same = float((ranks == fx["ranks"].astype(np.int64)).mean())
    print(f"\n[trained, fp16-fp8c] metric drift {np.round(drift, 8)}; scores: max abs diff {err.max():.3e} "
          f"(max |score| {np.abs(ref).max():.2f}); vs fp16x3 max abs diff {np.abs(scores - base).max():.3e}; ranks equal {same:.5f}")
    assert drift.max() <= 1e-4, drift
    assert err.max() <= 2e-5 * np.abs(ref).max(), err.max()
    assert same >= 0.999, same
    with enc.launch_options(live_rows=False):
        util.prepare_news_side(enc, dc, 1024)
        every = util.score_rows(model, dc, 0, dc.rows, 1024).cpu().numpy()
    util.prepare_news_side(enc, dc, 1024)
    listed = util.score_rows(model, dc, 0, dc.rows, 1024).cpu().numpy()
    np.testing.assert_array_equal(listed, every)
    np.testing.assert_array_equal(listed, scores)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["devset_tiny.npz", "devset_default.npz", "devset_large.npz", "devset_stress.npz"])
def test_fp16_fp8c_on_the_pinned_devsets(name):
    """The small dev sets (24 / 200 impressions) and the N = 26 / 65 news-graph shapes (devset_large / devset_stress) under
    "fp16-fp8c": metrics within 1e-4 of the reference's."""
    from test_hip_parity import DEVSETS
    from digat_amd import synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    fx = load_golden(name)
    spec = synthetic.SynthSpec(**DEVSETS[name])
    corpus = synthetic.make_corpus(spec)
    L = int(fx["depth"])
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, L, seed=spec.seed + 1, bias_std=0.05)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=L, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model = model.to(DEV).eval()
    model.graph_encoder.projection_mode = "fp16-fp8c"
    dc = util.DeviceCorpus.from_numpy(corpus, torch.device(DEV))
    scores, metrics = util.compute_scores(model, dc, 1024, labels=corpus.row_label)
    ref = fx["scores"]
    print(f"\n[{name} fp16-fp8c] max rel score diff {np.max(np.abs(scores - ref) / (np.abs(ref) + 1e-3)):.3e}")
    np.testing.assert_allclose(metrics, fx["metrics"], rtol=0, atol=1e-4)


@pytest.mark.gpu
def test_fp16_fp8c_out_of_range_activation_raises():
    """fp16x3's range applies (x_hi is the same fp16 piece): deep-layer features past |x| = 4094 raise the device flag, and an
    explicit "fp16-fp8c" refuses to return such scores, as an explicit "fp16x3" does."""
    from digat_amd import _lib, synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    d = 400
    spec = synthetic.SynthSpec(news_num=384, sag_neighbors=3, sag_hops=2, max_history_num=50, category_num=17, embedding_dim=d,
                               impressions=64, seed=5, embedding_scale=8.0)
    corpus = synthetic.make_corpus(spec)
    state = synthetic.make_state_dict(d, spec.category_num, 3, seed=6, bias_std=0.05)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=3, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model = model.to(DEV).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, torch.device(DEV))
    enc = model.graph_encoder
    with torch.no_grad():
        for g in ("news", "user"):
            getattr(enc, f"{g}_graph_attention_W")[0].weight.mul_(300.0)
    enc.projection_mode = "fp16-fp8c"
    with pytest.raises(_lib.DigatHipError, match="fp16-fp8c"):
        util.compute_scores(model, dc, 1024, labels=corpus.row_label)


def test_f16f8c_kernel_runs_the_scaled_fp8_mfma():
    """The evidence that the fp8 matrix cores run: the new kernel's code holds v_mfma_scale_f32_16x16x128_f8f6f4."""
    from digat_amd import _lib
    objdump = "/opt/rocm/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.fail("llvm-objdump not found under /opt/rocm/llvm/bin")
    import glob
    import shutil
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        # --offloading writes the embedded device code objects next to its input: work on a copy
        lib = os.path.join(tmp, "lib.so")
        shutil.copyfile(_lib.LIB_PATH, lib)
        subprocess.run([objdump, "--offloading", lib], check=True, capture_output=True, cwd=tmp)
        cos = [p for p in glob.glob(os.path.join(tmp, "lib.so.*")) if "gfx950" in p]
        assert cos, "no gfx950 code object in the library"
        text = subprocess.run([objdump, "-d", cos[0]], check=True, capture_output=True, text=True).stdout
    blocks, cur = {}, None
    for line in text.splitlines():
        if line.endswith(">:") and "<" in line:
            cur = line[line.index("<") + 1:-2]
            blocks[cur] = []
        elif cur is not None:
            blocks[cur].append(line)
    names = [n for n in blocks if "gemm_f16f8c_kernel" in n]
    assert names, "the fp16-fp8c kernel is not in the library"
    for n in names:
        assert any("v_mfma_scale_f32_16x16x128_f8f6f4" in l for l in blocks[n]), n
