"""CPU suite: listwise distillation without a GPU — the list-softmax entries are declared, exported, bound and refuse bad arguments
before any launch; the float64 host contracts (``evaluate.list_softmax_host`` / ``_grad_host`` / ``_keys_host``, which the GPU suite
holds the kernels to) against an independent ``torch.autograd`` composition and against ``pool_softmax_host`` where the two losses
coincide; and ``util.score_lists``, ``nrms.distil_step``, ``distil_retriever``, ``impression_lists`` and ``teacher_agreement`` on CPU
tensors through the stock route."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import list_softmax_common as LC
import nrms_common as NC
import pool_softmax_common as PC
from conftest import REPO

OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3
NEW = ("digat_list_softmax_workspace_bytes", "digat_list_softmax_fwd", "digat_list_softmax_bwd")
KERNELS = ("lsm_fwd_kernel", "lsm_users_kernel", "lsm_rows_kernel")
FIXTURE = "nrms_train_tiny.npz"


def test_new_symbols_are_declared_exported_and_bound():
    from digat_amd import _lib, build, evaluate
    build.build(verbose=False)
    header = open(os.path.join(REPO, "include", "digat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/digat_hip.h"
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.digat_version() == _lib.ABI_VERSION == 4
    assert int(re.search(r"#define\s+DIGAT_LIST_SOFTMAX_MAX_D\s+(\d+)", header).group(1)) == evaluate.LIST_SOFTMAX_MAX_D == 512
    kernels = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    assert kernels.index('#include "digat_pool_softmax.inc"') < kernels.index('#include "digat_list_softmax.inc"')
    assert L.digat_list_softmax_workspace_bytes(5, 7) == 256 and L.digat_list_softmax_workspace_bytes(4096, 1024) == 4096 * 1024 * 4
    assert L.digat_list_softmax_workspace_bytes(-1, 7) == 0


def test_the_resource_table_says_scratch_zero_for_every_kernel():
    text = open(os.path.join(REPO, "digat_amd", "csrc", "digat_list_softmax.inc")).read()
    head = text[:text.index("#define")]
    for k in KERNELS:
        line = [l for l in head.splitlines() if re.match(r"//\s+%s\s+VGPRs \d+" % k, l)]
        assert len(line) == 1 and "scratch 0" in line[0] and re.search(r"LDS \d+ B", line[0]), k
        assert re.search(r"__global__ void __launch_bounds__\(256\) %s\(" % k, text), k
    assert "atomic" not in text[text.index("#define"):], "no atomics, floating-point or other, in the list-softmax kernels"


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)

    def fwd(users=p, rows=p, ids=p, count=p, teacher=p, G=3, P=5, M=4, d=8, scale=1.0, temperature=1.0, o_loss=p, o_lse=p, o_valid=p,
            o_scores=p):
        return L.digat_list_softmax_fwd(users, rows, ids, count, teacher, G, P, M, d, scale, temperature, o_loss, o_lse, o_valid, o_scores,
                                        None)

    def bwd(users=p, rows=p, ids=p, count=p, teacher=p, G=3, P=5, M=4, d=8, scale=1.0, temperature=1.0, lse=p, scores=p, gl=p, keys=p, E=2,
            d_users=p, d_rows=p, ws=p, ws_bytes=256):
        return L.digat_list_softmax_bwd(users, rows, ids, count, teacher, G, P, M, d, scale, temperature, lse, scores, gl, keys, E, d_users,
                                        d_rows, ws, ws_bytes, None)
    for call in (fwd, bwd):
        assert call(M=0) == SHAPE and call(M=1025) == SHAPE and call(d=513) == SHAPE and call(d=0) == SHAPE
        assert call(temperature=0.0) == ARG and call(temperature=-1.0) == ARG and call(temperature=float("nan")) == ARG
        assert call(temperature=float("inf")) == ARG
        for name in ("users", "rows", "ids", "teacher"):
            assert call(**{name: None}) == ARG, name
        assert call(G=-1) == ARG and call(P=-1) == ARG
        assert call(G=1 << 21, M=1024) == SHAPE                    # G M = 2^31
    for name in ("o_loss", "o_lse", "o_valid", "o_scores"):
        assert fwd(**{name: None}) == ARG, name
    for name in ("lse", "scores", "gl", "d_users", "ws"):
        assert bwd(**{name: None}) == ARG, name
    assert bwd(keys=None) == ARG and bwd(E=-1) == ARG and bwd(E=13) == ARG          # more entries than slots
    assert bwd(ws_bytes=255) == WORKSPACE
    assert fwd(G=0) == OK                                          # nothing to do: no launch
    assert fwd(G=0, count=None) == OK


# ---------------------------------------------------------------------------------------------------------------------
# the host contracts against an independent float64 composition
# ---------------------------------------------------------------------------------------------------------------------
CASES = ((1, 1, 3), (2, 5, 4), (7, 9, 6), (9, 33, 5), (12, 3, 2))


def _host(users, rows, ids, count, teacher, scale, temperature, gl):
    from digat_amd import evaluate
    S = np.nan_to_num(LC.stock_fp64(users, rows, ids, count, teacher)[3])              # the stock scores; no-element slots hold anything
    loss, lse, valid = evaluate.list_softmax_host(S, ids, count, teacher, len(rows), scale, temperature)
    dU, dR = evaluate.list_softmax_grad_host(users, rows, S, ids, count, teacher, scale, temperature, gl)
    return loss, lse, valid, dU, dR, evaluate.list_softmax_keys_host(ids, count, len(rows))


def _close(got, want, what, rtol=1e-12, floor=0.0):
    """``rtol`` of the larger of an entry's size, the array's largest entry, and ``floor`` — the size of the sums a
    gradient that is identically zero (a list of one element) is the difference of."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(got[~np.isfinite(got)], want[~np.isfinite(want)], equal_nan=True), what
    fin = np.isfinite(want)
    scale = max(np.abs(want[fin]).max() if fin.any() else 0.0, floor)
    assert (np.abs(got[fin] - want[fin]) <= rtol * np.maximum(np.abs(want[fin]), scale) + 1e-300).all(), (what, np.abs(got[fin] - want[fin]).max())


@pytest.mark.parametrize("G,M,d", CASES)
def test_host_contracts_against_the_stock_composition(G, M, d):
    rng = np.random.default_rng(100 * G + M)
    for scale, temperature, counted in ((1.0, 1.0, True), (0.7, 2.5, True), (1.3, 0.05, False)):
        users, rows, ids, count, teacher = LC.case(rng, G, M, d, bad=0.15)
        cnt = count if counted else None
        gl = rng.standard_normal(G)
        w_loss, w_lse, w_valid, _, w_dU, w_dR, w_keys = LC.stock_fp64(users, rows, ids, cnt, teacher, scale, temperature, gl)
        loss, lse, valid, dU, dR, keys = _host(users, rows, ids, cnt, teacher, scale, temperature, gl)
        what = (G, M, d, scale, temperature)
        assert np.array_equal(valid, w_valid) and np.array_equal(keys, w_keys), what
        assert (loss[~valid] == 0).all() and (loss[valid] >= -1e-12).all(), what
        _close(lse, w_lse, f"{what} lse")
        _close(loss, w_loss, f"{what} loss", rtol=1e-10)
        _close(dU, w_dU, f"{what} d_users", rtol=1e-10, floor=LC.cancelled(gl, scale, rows))
        _close(dR, w_dR, f"{what} d_rows", rtol=1e-10, floor=LC.cancelled(gl, scale, users))


def test_the_special_lists_are_what_they_should_be():
    """ids out of range and negative, counts 0, negative and above M, a repeated id inside a list and across lists, teacher rows that
    are all -inf, one-hot, or hold a NaN and a +inf: each is met, and means what the contract says."""
    from digat_amd import evaluate
    rng = np.random.default_rng(4)
    G, M, d = 9, 6, 4
    users, rows, ids, count, teacher = LC.case(rng, G, M, d, bad=0.2)
    P = len(rows)
    assert (ids < 0).any() and (ids >= P).any() and 0 in count and (count < 0).any() and (count > M).any()
    assert (ids[:, 0] == ids[:, 1]).any() and len(np.unique(ids[(ids >= 0) & (ids < P)])) < ((ids >= 0) & (ids < P)).sum()
    assert np.isneginf(teacher[0]).all() and np.isfinite(teacher[1]).sum() == 1 and np.isnan(teacher[2, 0]) and np.isposinf(teacher[2, -1])
    ids[1, 2] = 1                                                   # the one-hot row's hot slot is an element
    S = np.nan_to_num(LC.stock_fp64(users, rows, ids, count, teacher)[3])
    loss, lse, valid = evaluate.list_softmax_host(S, ids, count, teacher, P)
    by = {int(c): g for g, c in enumerate(count)}
    assert not valid[by[0]] and np.isneginf(lse[by[0]]) and not valid[by[-3]] and np.isneginf(lse[by[-3]])
    assert not valid[0] and np.isfinite(lse[0]) and loss[0] == 0, "elements but no mass"
    x = np.where((ids[1] >= 0) & (ids[1] < P), S[1], -np.inf)
    assert valid[1] and abs(loss[1] - (lse[1] - x[2])) <= 1e-12 * abs(lse[1]), "a one-hot teacher is the click loss"
    t2 = teacher.copy()
    t2[2, 0], t2[2, -1] = -np.inf, -np.inf
    assert np.array_equal(evaluate.list_softmax_host(S, ids, count, t2, P)[0], loss), "NaN and +inf carry no mass, as -inf"
    over = evaluate.list_softmax_host(S, ids, np.where(count > M, M, count), teacher, P)
    assert np.array_equal(over[0], loss) and np.array_equal(over[1], lse), "a count above M is M"
    with pytest.raises(ValueError, match="temperature"):
        evaluate.list_softmax_host(S, ids, count, teacher, P, temperature=0.0)
    with pytest.raises(ValueError, match="ids must be"):
        evaluate.list_softmax_host(S, ids[:, :3], count, teacher, P)


def test_a_list_of_one_element_has_a_gradient_that_is_identically_zero():
    """softmax over one element is 1 whatever the vectors are: p = q = 1.  The float64 contract gives exactly 0; the CPU route of
    ``evaluate.list_softmax`` — stock autograd, a difference of two equal sums — is held as ``_close_grad`` holds the pool of one: at
    2e-4 of the size of what cancels."""
    from digat_amd import evaluate
    rng = np.random.default_rng(8)
    G, M, d = 4, 5, 6
    users, rows, ids, _, teacher = LC.case(rng, G, M, d, bad=0.0)
    count = np.ones(G, dtype=np.int32)
    gl = rng.standard_normal(G)
    S = np.nan_to_num(LC.stock_fp64(users, rows, ids, count, teacher)[3])
    loss, lse, valid = evaluate.list_softmax_host(S, ids, count, teacher, len(rows))
    dU, dR = evaluate.list_softmax_grad_host(users, rows, S, ids, count, teacher, grad_loss=gl)
    assert valid.all() and (loss == 0).all() and (dU == 0).all() and (dR == 0).all()
    U, R = torch.from_numpy(users).requires_grad_(True), torch.from_numpy(rows).requires_grad_(True)
    got = evaluate.list_softmax(U, R, torch.from_numpy(ids), torch.from_numpy(count), torch.from_numpy(teacher))
    (got[0] * torch.from_numpy(gl).float()).sum().backward()
    assert float(got[0].detach().abs().max()) <= 1e-6
    assert float(U.grad.abs().max()) <= 2e-4 * LC.cancelled(gl, 1.0, rows) and float(R.grad.abs().max()) <= 2e-4 * LC.cancelled(gl, 1.0, users)


def test_anchor_the_whole_pool_with_a_one_hot_teacher_is_the_pool_softmax():
    from digat_amd import evaluate
    rng = np.random.default_rng(21)
    G, P, d, scale = 6, 40, 7, 0.8
    users, news, _, _ = PC.case(rng, G, P, d, False, False)
    S = users.astype(np.float64) @ news.astype(np.float64).T
    pos = rng.integers(0, P, size=G).astype(np.int64)
    start = np.arange(G + 1, dtype=np.int64)
    gl = rng.standard_normal(G)
    p_loss, p_lse, ranked = evaluate.pool_softmax_host(S, pos, start, scale=scale)
    p_dU, p_dR = evaluate.pool_softmax_grad_host(users, news, S, pos, start, scale=scale, grad_loss=gl)
    ids = np.repeat(np.arange(P, dtype=np.int64)[None, :], G, axis=0)
    teacher = np.full((G, P), -np.inf)
    teacher[np.arange(G), pos] = 0.0
    loss, lse, valid = evaluate.list_softmax_host(S, ids, None, teacher, P, scale, 1.0)
    dU, dR = evaluate.list_softmax_grad_host(users, news, S, ids, None, teacher, scale, 1.0, gl)
    assert ranked.all() and valid.all()
    _close(lse, p_lse, "lse")
    _close(loss, p_loss, "loss")
    _close(dU, p_dU, "d_users", rtol=1e-11)
    _close(dR, p_dR, "d_rows", rtol=1e-11)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_cpu_path_of_list_softmax_agrees_with_the_host_and_is_differentiable(dtype):
    from digat_amd import evaluate
    rng = np.random.default_rng(3)
    G, M, d = 9, 12, 5
    users, rows, ids, count, teacher = LC.case(rng, G, M, d, bad=0.15)
    gl = rng.standard_normal(G)
    U, R = torch.from_numpy(users).to(dtype).requires_grad_(True), torch.from_numpy(rows).to(dtype).requires_grad_(True)
    Tt = torch.from_numpy(teacher).requires_grad_(True)
    loss, lse, scores = evaluate.list_softmax(U, R, torch.from_numpy(ids), torch.from_numpy(count), Tt, scale=0.6, temperature=1.7)
    assert loss.shape == lse.shape == (G,) and scores.shape == (G, M) and loss.dtype == dtype
    assert loss.requires_grad and not lse.requires_grad and not scores.requires_grad
    (loss * torch.from_numpy(gl).to(dtype)).sum().backward()
    assert Tt.grad is None, "no gradient to the teacher"
    w_loss, w_lse, w_valid, w_S, w_dU, w_dR, _ = LC.stock_fp64(users, rows, ids, count, teacher, 0.6, 1.7, gl)
    assert np.array_equal(np.isnan(scores.numpy()), np.isnan(w_S))
    rtol = 1e-10 if dtype == torch.float64 else 2e-4
    _close(scores.detach().numpy(), w_S, "scores", rtol=max(rtol, 1e-10))
    _close(lse.numpy(), w_lse, "lse", rtol=rtol)
    _close(loss.detach().numpy(), w_loss, "loss", rtol=rtol)
    _close(U.grad.numpy(), w_dU, "d_users", rtol=rtol, floor=LC.cancelled(gl, 0.6, rows))
    _close(R.grad.numpy(), w_dR, "d_rows", rtol=rtol, floor=LC.cancelled(gl, 0.6, users))
    for bad, match in (((U[:, :3], R, torch.from_numpy(ids), None, Tt), "share d"), ((U, R, torch.from_numpy(ids).float(), None, Tt), "ids must be"),
                       ((U, R, torch.from_numpy(ids), torch.from_numpy(count[:3]), Tt), "count must be"),
                       ((U, R, torch.from_numpy(ids), None, Tt[:, :3]), "teacher must be"),
                       ((U, R, torch.zeros((G, 1025), dtype=torch.int64), None, torch.zeros(G, 1025)), "SHORTLIST_MAX_K"),
                       ((torch.zeros(G, 513), torch.zeros(4, 513), torch.from_numpy(ids), None, Tt), "LIST_SOFTMAX_MAX_D")):
        with pytest.raises(ValueError, match=match):
            evaluate.list_softmax(*bad)
    with pytest.raises(ValueError, match="temperature"):
        evaluate.list_softmax(U, R, torch.from_numpy(ids), None, Tt, temperature=0.0)


def test_the_bound_is_inside_the_output_tolerance_at_the_largest_list():
    """The header's claim: at M = 1024 and |x|, |tau| <= 30 the derived bound lies inside atol 2e-6, rtol 1e-5 for every lse and loss."""
    from digat_amd import evaluate
    lse = np.linspace(-30.0, 37.0, 2001)
    assert (evaluate.list_softmax_bound(lse, 30.0, 30.0) <= 2e-6 + 1e-5 * np.abs(lse)).all()
    loss = np.r_[0.0, np.logspace(-9, np.log10(70.0), 4000)]
    assert (evaluate.list_softmax_bound(None, 30.0, 30.0, loss=loss) <= 2e-6 + 1e-5 * loss).all()


# ---------------------------------------------------------------------------------------------------------------------
# the callers on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_score_lists_fills_and_refusals(monkeypatch):
    """``util.score_lists`` with the scoring pass replaced by a function of the pair (the pass itself needs a GPU): every slot holds
    its own pair's score, ``-inf`` beyond ``count`` and at ids outside the corpus, whatever the chunking."""
    import types
    from digat_amd import util
    N, I, H = 50, 7, 4
    rng = np.random.default_rng(0)
    dc = util.DeviceCorpus.__new__(util.DeviceCorpus)
    dc.history = torch.from_numpy(rng.integers(0, N, size=(I, H)))
    dc.user_category_indices = torch.zeros((I, H), dtype=torch.int64)
    dc.user_graph = dc.user_category_mask = None
    dc.news_embedding = torch.zeros((N, 3))
    calls = []

    def fake_scoring(model, dc_, hist, cat, graph, mask, batch_size):
        def score(g0, g1, row_user, row_cand):
            calls.append((g0, g1, len(row_user)))
            return (1000.0 * row_user + row_cand).float()
        return (lambda: calls.append("prepare")), score
    monkeypatch.setattr(util, "recommend_scoring", fake_scoring)
    users = np.array([3, 0, 6, 2])
    ids = rng.integers(0, N, size=(4, 6)).astype(np.int64)
    ids[0, 1], ids[2, 5], ids[1, 0] = -1, N, N + 3
    count = np.array([6, 0, 9, 3])
    for max_rows in (util.RECOMMEND_MAX_ROWS, 4):
        calls.clear()
        got = util.score_lists(types.SimpleNamespace(), dc, users, ids, count, max_rows=max_rows)
        assert got.shape == (4, 6) and got.dtype == torch.float32 and calls[0] == "prepare"
        for g in range(4):
            for j in range(6):
                inside = j < min(max(count[g], 0), 6) and 0 <= ids[g, j] < N
                assert float(got[g, j]) == (1000.0 * g + ids[g, j] if inside else float("-inf")), (g, j)
        assert sum(c[2] for c in calls[1:]) == 5 + 0 + 5 + 3 and (len(calls) > 2) == (max_rows == 4)
    assert torch.equal(util.score_lists(types.SimpleNamespace(), dc, users, ids)[0, :1], torch.tensor([ids[0, 0]], dtype=torch.float32))
    with pytest.raises(ValueError, match="ids must be"):
        util.score_lists(None, dc, users, ids[:3], count)
    with pytest.raises(ValueError, match="ids must be"):
        util.score_lists(None, dc, users, ids.astype(np.float32), count)
    with pytest.raises(ValueError, match="count must have"):
        util.score_lists(None, dc, users, ids, count[:2])
    with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
        util.score_lists(None, dc, users, np.zeros((4, 1025), dtype=np.int64))
    with pytest.raises(ValueError, match="impression indices"):
        util.score_lists(None, dc, np.array([I]), ids[:1])


def _train_set(device="cpu"):
    """The training fixture's impressions with the first candidate of each clicked (test_hip_pool_softmax.py's)."""
    dev = NC.dev_set(FIXTURE, device)
    U, K = NC.case(FIXTURE)[2]["candidate_ids"].shape
    dev.row_label = (np.arange(U * K) % K == 0).astype(np.int64)
    return dev, U, K


def test_impression_lists_are_the_impressions():
    from digat_amd import nrms
    dev, U, K = _train_set()
    users, ids, teacher, count = nrms.impression_lists(dev)
    cand = NC.case(FIXTURE)[2]["candidate_ids"]
    assert np.array_equal(users, np.arange(U)) and np.array_equal(ids, cand) and (count == K).all() and count.dtype == np.int32
    assert (teacher[:, 0] == 0).all() and np.isneginf(teacher[:, 1:]).all() and teacher.dtype == np.float32
    # ragged impressions, some without a click: the rows of every impression in row order, -1 and -inf behind them
    dev.row_impression = np.array([0, 0, 0, 2, 2, 1, 3, 3, 3, 3])
    dev.row_candidate = np.array([5, 6, 7, 8, 9, 4, 1, 2, 3, 1])
    dev.row_label = np.array([0, 1, 1, 0, 0, 1, 0, 0, 0, 1])
    users, ids, teacher, count = nrms.impression_lists(dev)
    assert users.tolist() == [0, 1, 3] and count.tolist() == [3, 1, 4]
    assert ids.tolist() == [[5, 6, 7, -1], [4, -1, -1, -1], [1, 2, 3, 1]]
    assert np.array_equal(np.isfinite(teacher), np.array([[0, 1, 1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], dtype=bool))
    assert nrms.impression_lists(dev, users=np.array([2]))[2].tolist() == [[-np.inf, -np.inf]]


@pytest.mark.parametrize("pre", list(NC.MODELS))
def test_distil_step_on_an_impression_with_one_click_is_the_listwise_click_loss(pre):
    from digat_amd import nrms
    dev, U, K = _train_set()
    m = PC.double_twin(NC.model(FIXTURE, pre)).eval()
    lists = nrms.impression_lists(dev)
    g = 2
    loss = nrms.distil_step(m, dev, lists[0][g:g + 1], lists[1][g:g + 1], lists[2][g:g + 1], lists[3][g:g + 1])
    cand = torch.from_numpy(lists[1][g])
    sa = pre == "sa"
    with torch.no_grad():
        news = m.news_encoder.forward_stock(dev.title_text[cand][None], dev.title_mask[cand][None],
                                            dev.augmented_title_text[cand][None] if sa else None,
                                            dev.augmented_title_mask[cand][None] if sa else None)[0]
        hist = dev.history_ids[g:g + 1].to(torch.int64)
        user = m.user_encoder.forward_stock(dev.title_text[hist], dev.title_mask[hist], dev.history_mask[g:g + 1])[0]
        want = -torch.log_softmax(news @ user, dim=0)[0]
    assert loss.requires_grad and abs(float(loss.detach()) - float(want)) <= 1e-10 * abs(float(want))
    # a batch: the mean over the valid lists; a list without mass or without an element is not counted
    teacher = lists[2].copy()
    teacher[1] = -np.inf
    count = lists[3].copy()
    count[3] = 0
    all_ = nrms.distil_step(m, dev, lists[0], lists[1], teacher, count)
    each = [float(nrms.distil_step(m, dev, lists[0][i:i + 1], lists[1][i:i + 1], teacher[i:i + 1], count[i:i + 1]).detach()) for i in range(U)]
    assert each[1] == 0 and each[3] == 0 and abs(float(all_.detach()) - sum(each) / (U - 2)) <= 1e-10 * abs(float(all_.detach()))
    nothing = nrms.distil_step(m, dev, lists[0][:2], lists[1][:2], teacher[:2], np.zeros(2, dtype=np.int32))
    assert float(nothing.detach()) == 0
    nothing.backward()
    with pytest.raises(ValueError, match="teacher must be"):
        nrms.distil_step(m, dev, lists[0], lists[1], teacher[:, :2], count)
    with pytest.raises(ValueError, match="impression indices"):
        nrms.distil_step(m, dev, lists[0] + U, lists[1], teacher, count)
    with pytest.raises(ValueError, match="ids must be"):
        nrms.distil_step(m, dev, lists[0], lists[1][:2], teacher, count)


STEPS, SEED = 8, 5


def _mean_kl(m, dev, lists):
    from digat_amd import nrms
    m.eval()
    with torch.no_grad():
        return float(nrms.distil_step(m, dev, *lists[:3], lists[3], temperature=2.0))


def test_distil_retriever_lowers_the_mean_kl_of_its_lists():
    """A direction check with no threshold: float64 CPU copy, dropout 0, fixed seed — the mean KL over the fixed lists in eval mode is
    lower after the steps than before."""
    from digat_amd import nrms
    dev, U, K = _train_set()
    rng = np.random.default_rng(SEED)
    N = int(dev.title_text.shape[0])
    M = 6
    ids = np.stack([rng.permutation(np.arange(1, N))[:M] for _ in range(U)]).astype(np.int64)
    teacher = rng.standard_normal((U, M)).astype(np.float32) * 2
    count = np.full(U, M, dtype=np.int32)
    count[0] = M - 2
    lists = (np.arange(U), ids, teacher, count)
    m = PC.double_twin(NC.model(FIXTURE, "nrms"))
    before = _mean_kl(m, dev, lists)
    losses = nrms.distil_retriever(m, dev, lists, STEPS, batch_users=3, lr=1e-3, seed=SEED, temperature=2.0)
    after = _mean_kl(m, dev, lists)
    print("mean KL before", before, "after", after, "step losses", losses)
    assert len(losses) == STEPS and all(np.isfinite(losses))
    assert after < before
    again = PC.double_twin(NC.model(FIXTURE, "nrms"))
    assert nrms.distil_retriever(again, dev, lists, 2, batch_users=3, lr=1e-3, seed=SEED, temperature=2.0) == losses[:2], "seeded draws"
    with pytest.raises(ValueError, match="lists must be"):
        nrms.distil_retriever(m, dev, lists[:3], 1)
    with pytest.raises(ValueError, match="no list"):
        nrms.distil_retriever(m, dev, (lists[0][:0], ids[:0], teacher[:0], count[:0]), 1)


def test_teacher_agreement_counts_the_teachers_top_k_in_the_students_list():
    from digat_amd import evaluate, nrms
    student = np.array([[5, 6, 7, 8], [1, 2, 3, 4], [9, 9, 9, 9], [4, 3, 2, 1]])
    s_count = np.array([4, 2, 0, 4])
    teacher = np.array([[7, 1, 5, 2], [3, 2, 1, 9], [9, 1, 2, 3], [7, 7, 7, 7]])
    t_count = np.array([4, 3, 4, 0])
    got = nrms.teacher_agreement(student, s_count, teacher, t_count, ks=(1, 2, 10))
    want = np.array([[1.0, 0.5, 0.5], [0.0, 0.5, 2.0 / 3.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    assert got["names"] == ["agreement@1", "agreement@2", "agreement@10"] and np.array_equal(got["per_user"], want)
    for c, name in enumerate(got["names"]):
        assert got[name] == want[:, c].mean()
    iv = evaluate.metric_intervals(got["per_user"], names=got["names"], replicates=50)      # the per-user matrix goes in unchanged
    assert set(got["names"]) <= set(iv) or all(n in str(iv) for n in got["names"])
    assert nrms.teacher_agreement(student, None, teacher, None, ks=(4,))["per_user"][:, 0].tolist() == [0.5, 0.75, 0.25, 0.0]
    with pytest.raises(ValueError, match="positive integer"):
        nrms.teacher_agreement(student, s_count, teacher, t_count, ks=(0,))
    with pytest.raises(ValueError, match="student_ids must be"):
        nrms.teacher_agreement(student[:2], s_count[:2], teacher, t_count)
