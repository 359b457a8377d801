"""GPU suite: the fused per-user list softmax (``digat_list_softmax_fwd`` / ``_bwd``, ``evaluate.list_softmax``), ``nrms.distil_step``
and ``util.score_lists`` on it.  What is a matter of bits — the scores, which slots are elements, which lists are valid, that two
calls and a list alone or in a batch agree — is held exactly; ``lse`` and ``loss`` to the float64 host contract on the kernel's own
scores (``digat_dot_scores`` gathered at the list's ids) at the bound the kernel file derives; the gradients at the training
tolerance 2e-4."""
import functools
import types

import numpy as np
import pytest
import torch

import list_softmax_common as LC
import nrms_common as NC
import pool_softmax_common as PC
from nrms_common import close

pytestmark = pytest.mark.gpu

# G in {1, 3, 65}, M in {1, 63, 65, 255, 257, 1024}, d in {1, 5, 36, 400, 512}
SWEEP = ((1, 1, 1), (3, 63, 5), (65, 65, 36), (1, 255, 400), (3, 257, 512), (65, 1024, 5), (3, 1024, 400), (65, 255, 1), (1, 1024, 512),
         (65, 63, 400), (3, 65, 36), (1, 257, 36))
SLAB = 256      # csrc/digat_list_softmax.inc: LSM_SLAB, the slots one pass of the forward scores — one per thread


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).view(np.uint32)


def test_the_sweep_covers_what_it_should():
    from digat_amd import evaluate
    assert {g for g, _, _ in SWEEP} == {1, 3, 65}                                         # one list, a few, more than a wave of them
    assert {m for _, m, _ in SWEEP} == {1, 63, 65, SLAB - 1, SLAB + 1, evaluate.SHORTLIST_MAX_K}       # wave, slab, the longest list
    assert {d for _, _, d in SWEEP} == {1, 5, 36, 400, evaluate.LIST_SOFTMAX_MAX_D}       # scalar loads, one staged block + 4, the flagship
    assert len(SWEEP) == 12


def _raw_forward(users, rows, ids, count, teacher, scale, temperature):
    """The C entry itself, into buffers with a guard behind them: ``(loss, lse, valid, scores)`` as numpy."""
    from digat_amd import _lib
    G, M = ids.shape
    f = dict(dtype=torch.float32, device=_dev())
    U, R, I, Cn, Tt = _t(users), _t(rows), _t(ids), _t(count), _t(teacher)
    loss, lse, sc = torch.full((G + 4,), 77.0, **f), torch.full((G + 4,), 77.0, **f), torch.full((G * M + 4,), 77.0, **f)
    valid = torch.full((G + 4,), 77, dtype=torch.int32, device=_dev())
    _lib.check(_lib.lib().digat_list_softmax_fwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), _lib.ptr(Cn), Tt.data_ptr(), G, len(rows), M,
                                                 users.shape[1], scale, temperature, loss.data_ptr(), lse.data_ptr(), valid.data_ptr(),
                                                 sc.data_ptr(), _lib.stream_ptr()), "digat_list_softmax_fwd")
    assert (loss[G:] == 77).all() and (lse[G:] == 77).all() and (valid[G:] == 77).all() and (sc[G * M:] == 77).all(), "nothing beyond the arrays"
    return loss[:G].cpu().numpy(), lse[:G].cpu().numpy(), valid[:G].cpu().numpy(), sc[:G * M].view(G, M).cpu().numpy()


def _run(users, rows, ids, count, teacher, scale, temperature, gl):
    """One forward and backward through autograd on the device: ``(loss, lse, scores, d_users, d_rows)`` as numpy."""
    from digat_amd import evaluate
    U, R = _t(users).requires_grad_(True), _t(rows).requires_grad_(True)
    loss, lse, scores = evaluate.list_softmax(U, R, _t(ids), _t(count), _t(teacher), scale=scale, temperature=temperature)
    assert loss.dtype == lse.dtype == scores.dtype == torch.float32
    assert loss.shape == lse.shape == (len(users),) and scores.shape == ids.shape
    assert loss.requires_grad and not lse.requires_grad and not scores.requires_grad
    (loss * _t(gl)).sum().backward()
    return tuple(t.detach().cpu().numpy() for t in (loss, lse, scores, U.grad, R.grad))


def _close_grad(got, want, cancelled, what):
    """The training tolerance, ``close(rtol=2e-4, atol=0)``: relative to the gradient's own size.  Where the exact gradient is
    IDENTICALLY zero — lists of one element: p = q = 1 whatever the vectors are — it has no size of its own and is held at the same
    rtol to the size ``cancelled`` of the two equal sums it is the difference of (test_hip_pool_softmax.py's rule)."""
    if np.abs(want).max() > 0:
        close(torch.from_numpy(got), want, what, rtol=2e-4, atol=0.0)
    else:
        assert np.isfinite(got).all() and np.abs(got).max() <= 2e-4 * cancelled, (what, float(np.abs(got).max()), cancelled)


def _gathered(users, rows, ids):
    """``dot_scores`` at the lists' ids: [G, M] float32, 0 where the id is no row."""
    from digat_amd import evaluate
    S = evaluate.dot_scores(_t(users), _t(rows)).cpu().numpy()
    ok = (ids >= 0) & (ids < len(rows))
    return np.where(ok, S[np.arange(len(ids))[:, None], np.where(ok, ids, 0)], np.float32(0))


def _check(users, rows, ids, count, teacher, scale, temperature, rng, what):
    """The whole contract of one call against the host functions on ``dot_scores``.  ``scale`` and ``temperature`` are float32 numbers."""
    from digat_amd import evaluate
    assert float(np.float32(scale)) == scale and float(np.float32(temperature)) == temperature
    G, M = ids.shape
    P = len(rows)
    gl = rng.standard_normal(G).astype(np.float32)
    loss, lse, scores, dU, dR = _run(users, rows, ids, count, teacher, scale, temperature, gl)
    r_loss, r_lse, r_valid, r_scores = _raw_forward(users, rows, ids, count, teacher, scale, temperature)
    for a, b, name in ((loss, r_loss, "loss"), (lse, r_lse, "lse"), (scores, r_scores, "scores")):
        assert np.array_equal(_bits(a), _bits(b)), (what, name, "the autograd function and the C entry")
    S = _gathered(users, rows, ids)
    cnt = np.full(G, M) if count is None else np.clip(count, 0, M)
    elem = (np.arange(M)[None, :] < cnt[:, None]) & (ids >= 0) & (ids < P)
    w_loss, w_lse, w_valid = evaluate.list_softmax_host(S, ids, count, teacher, P, scale, temperature)
    # bits
    assert np.array_equal(np.isnan(scores), ~elem), (what, "NaN exactly where the slot is no element")
    assert np.array_equal(_bits(scores[elem]), _bits(S[elem])), (what, "score bits")
    assert np.array_equal(r_valid, w_valid.astype(np.int32)), (what, "valid")
    assert (loss[~w_valid] == 0).all(), what
    # lse and loss at the derived bound
    none = np.isneginf(w_lse)
    assert np.array_equal(np.isneginf(lse), none), what
    x = np.where(elem, scale * S.astype(np.float64), 0.0)
    x_max = np.abs(x).max(axis=1)
    with np.errstate(invalid="ignore"):
        tau_max = np.abs(np.where(elem & np.isfinite(teacher), teacher.astype(np.float64) / temperature, 0.0)).max(axis=1)
    if (~none).any():
        b_lse = evaluate.list_softmax_bound(w_lse[~none], x_max[~none], tau_max[~none])
        err = np.abs(lse[~none] - w_lse[~none])
        print(what, "lse: worst error over bound", float((err / b_lse).max()), "largest bound", float(b_lse.max()))
        assert (err <= b_lse).all(), (what, float((err / b_lse).max()))
    if w_valid.any():
        b_loss = evaluate.list_softmax_bound(None, x_max[w_valid], tau_max[w_valid], loss=w_loss[w_valid])
        err = np.abs(loss[w_valid] - w_loss[w_valid])
        print(what, "loss: worst error over bound", float((err / b_loss).max()), "largest bound", float(b_loss.max()))
        assert (err <= b_loss).all(), (what, float((err / b_loss).max()))
    # gradients at the training tolerance
    w_dU, w_dR = evaluate.list_softmax_grad_host(users, rows, S, ids, count, teacher, scale, temperature, gl)
    _close_grad(dU, w_dU, LC.cancelled(gl, scale, rows), f"{what} d_users")
    _close_grad(dR, w_dR, LC.cancelled(gl, scale, users), f"{what} d_rows")
    named = np.zeros(P, dtype=bool)
    named[ids[elem]] = True
    assert (dR[~named] == 0).all() and (dU[~w_valid] == 0).all(), (what, "exactly zero where nothing contributes")
    return loss, lse, scores, dU, dR


@pytest.mark.parametrize("G,M,d", SWEEP)
def test_loss_and_gradients_against_the_host_contract(G, M, d):
    rng = np.random.default_rng(1000 * G + M + d)
    n = SWEEP.index((G, M, d))
    for counted in (True, False):
        users, rows, ids, count, teacher = LC.case(rng, G, M, d)
        _check(users, rows, ids, count if counted else None, teacher, 1.0 if n % 2 else 0.5, 2.0 if n % 3 else 1.0, rng, (G, M, d, counted))
        n += 1


def test_lists_of_one_element_have_a_zero_gradient():
    rng = np.random.default_rng(2)
    G, M, d = 5, 70, 36
    users, rows, ids, _, teacher = LC.case(rng, G, M, d, bad=0.0)
    loss, lse, scores, dU, dR = _check(users, rows, ids, np.ones(G, dtype=np.int32), teacher, 1.0, 1.0, rng, "one element")
    assert (np.abs(loss) <= 1e-6).all()


def test_two_calls_and_a_list_alone_give_the_same_bits():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(31)
    G, M, d = 65, 300, 36
    users, rows, ids, count, teacher = LC.case(rng, G, M, d)
    gl = rng.standard_normal(G).astype(np.float32)
    first = _run(users, rows, ids, count, teacher, 0.5, 2.0, gl)
    again = _run(users, rows, ids, count, teacher, 0.5, 2.0, gl)
    names = ("loss", "lse", "scores", "d_users", "d_rows")
    for a, b, name in zip(first, again, names):
        assert np.array_equal(_bits(a), _bits(b)), name
    # a list scored alone: the same bits as inside the batch of 65 (the gradient of the rows is another sum and is not compared)
    for g in (7, 64):
        one = _run(users[g:g + 1], rows, ids[g:g + 1], count[g:g + 1], teacher[g:g + 1], 0.5, 2.0, gl[g:g + 1])
        for k in range(4):
            assert np.array_equal(_bits(one[k][0]), _bits(first[k][g])), (g, names[k])
    # rows that no list names are exactly zero in a buffer pre-filled with NaN: every row is written, nothing beyond
    P = len(rows)
    f = dict(dtype=torch.float32, device=_dev())
    U, R, I, Cn, Tt = _t(users), _t(rows), _t(ids), _t(count), _t(teacher)
    loss, lse, scores = evaluate.list_softmax(U, R, I, Cn, Tt, scale=0.5, temperature=2.0)
    keys = _t(evaluate.list_softmax_keys_host(ids, count, P))
    d_users, d_rows = torch.full((G + 1, d), float("nan"), **f), torch.full((P + 1, d), float("nan"), **f)
    L = _lib.lib()
    need = int(L.digat_list_softmax_workspace_bytes(G, M))
    ws = _lib.workspace(need, _dev(), "list_softmax")
    ws.fill_(0xFF)
    GL = _t(gl)
    head = (U.data_ptr(), R.data_ptr(), I.data_ptr(), Cn.data_ptr(), Tt.data_ptr(), G, P, M, d, 0.5, 2.0, lse.data_ptr(), scores.data_ptr(),
            GL.data_ptr())
    _lib.check(L.digat_list_softmax_bwd(*head, keys.data_ptr(), int(keys.numel()), d_users.data_ptr(), d_rows.data_ptr(), ws.data_ptr(), need,
                                        _lib.stream_ptr()), "digat_list_softmax_bwd")
    assert torch.isnan(d_users[G]).all() and torch.isnan(d_rows[P]).all()
    assert np.array_equal(_bits(d_users[:G]), _bits(first[3])) and np.array_equal(_bits(d_rows[:P]), _bits(first[4]))
    cnt = np.clip(count, 0, M)
    elem = (np.arange(M)[None, :] < cnt[:, None]) & (ids >= 0) & (ids < P)
    named = np.zeros(P, dtype=bool)
    named[ids[elem]] = True
    assert (~named).any() and (d_rows[:P][_t(~named)] == 0).all()
    # without d_rows: one launch, no keys, the same d_users
    d_users.fill_(float("nan"))
    _lib.check(L.digat_list_softmax_bwd(*head, None, 0, d_users.data_ptr(), None, ws.data_ptr(), need, _lib.stream_ptr()), "digat_list_softmax_bwd")
    assert np.array_equal(_bits(d_users[:G]), _bits(first[3]))


def test_scores_and_teacher_values_of_three_hundred_stay_finite():
    """x and tau reach +-300: exp overflows (and underflows) unless the maximum is subtracted."""
    rng = np.random.default_rng(77)
    G, M, d = 5, 300, 32
    users, rows, ids, count, teacher = LC.case(rng, G, M, d, bad=0.05)
    count[:] = M
    S = users.astype(np.float64) @ rows.astype(np.float64).T
    scale = float(np.float32(300.0 / np.abs(S).max()))
    fin = np.isfinite(teacher)
    teacher[fin] *= np.float32(300.0 / np.abs(teacher[fin]).max())
    loss, lse, scores, dU, dR = _check(users, rows, ids, count, teacher, scale, 1.0, rng, "range")
    assert np.abs(lse).max() > 150 and np.isfinite(loss).all() and np.isfinite(dU).all() and np.isfinite(dR).all()


@pytest.mark.parametrize("temperature", [0.05, 20.0])
def test_temperatures(temperature):
    rng = np.random.default_rng(5)
    users, rows, ids, count, teacher = LC.case(rng, 9, 130, 20)
    _check(users, rows, ids, count, teacher, 1.0, float(np.float32(temperature)), rng, ("temperature", temperature))


def test_anchor_the_whole_pool_with_a_one_hot_teacher_is_pool_softmax():
    from digat_amd import evaluate
    rng = np.random.default_rng(21)
    G, P, d, scale = 6, 300, 36, 0.5
    users, news, _, _ = PC.case(rng, G, P, d, False, False)
    users *= np.float32(1.5 / np.sqrt(d))
    pos = rng.integers(0, P, size=G).astype(np.int64)
    start = np.arange(G + 1, dtype=np.int64)
    gl = rng.standard_normal(G).astype(np.float32)
    U, V = _t(users).requires_grad_(True), _t(news).requires_grad_(True)
    p_loss, p_lse, _ = evaluate.pool_softmax(U, V, _t(pos), start, scale=scale)
    (p_loss * _t(gl)).sum().backward()
    p_dU, p_dV = U.grad.cpu().numpy(), V.grad.cpu().numpy()
    ids = np.repeat(np.arange(P, dtype=np.int64)[None, :], G, axis=0)
    teacher = np.full((G, P), -np.inf, dtype=np.float32)
    teacher[np.arange(G), pos] = 0.0
    loss, lse, scores, dU, dR = _run(users, news, ids, None, teacher, scale, 1.0, gl)
    x = scale * _gathered(users, news, ids).astype(np.float64)
    x_max = np.abs(x).max(axis=1)
    p_loss, p_lse = p_loss.detach().cpu().numpy().astype(np.float64), p_lse.cpu().numpy().astype(np.float64)
    both = evaluate.list_softmax_bound(None, x_max, 0.0, loss=p_loss) + evaluate.pool_softmax_bound(P, p_lse, x_max, x[np.arange(G), pos], p_loss)
    assert (np.abs(loss - p_loss) <= both).all(), float((np.abs(loss - p_loss) / both).max())
    assert (np.abs(lse - p_lse) <= evaluate.list_softmax_bound(p_lse, x_max) + evaluate.pool_softmax_bound(P, p_lse, x_max)).all()
    close(torch.from_numpy(dU), p_dU, "d_users against pool_softmax", rtol=2e-4, atol=0.0)
    close(torch.from_numpy(dR), p_dV, "d_rows against pool_softmax", rtol=2e-4, atol=0.0)


def test_refusals_and_empty_calls():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(13)
    G, M, d = 4, 9, 8
    users, rows, ids, count, teacher = LC.case(rng, G, M, d)
    P = len(rows)
    U, R, I, Cn, Tt = _t(users), _t(rows), _t(ids), _t(count), _t(teacher)
    L = _lib.lib()
    f = dict(dtype=torch.float32, device=_dev())
    o = torch.full((4, G * M), 77.0, **f)
    valid = torch.full((G,), 77, dtype=torch.int32, device=_dev())

    def fwd(G=G, M=M, d=d, temperature=1.0):
        return L.digat_list_softmax_fwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), Cn.data_ptr(), Tt.data_ptr(), G, P, M, d, 1.0, temperature,
                                        o[0].data_ptr(), o[1].data_ptr(), valid.data_ptr(), o[2].data_ptr(), _lib.stream_ptr())
    assert fwd(M=0) == 2 and fwd(M=1025) == 2 and fwd(d=513) == 2 and fwd(temperature=0.0) == 1 and fwd(temperature=-2.0) == 1
    assert fwd(G=0) == 0
    torch.cuda.synchronize()
    assert (o == 77).all() and (valid == 77).all(), "a refused or empty call launches nothing"
    with pytest.raises(ValueError, match="temperature"):
        evaluate.list_softmax(U, R, I, Cn, Tt, temperature=0.0)
    with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
        evaluate.list_softmax(U, R, I[:, :0], Cn, Tt[:, :0])
    with pytest.raises(ValueError, match="one device"):
        evaluate.list_softmax(U, R, I.cpu(), Cn, Tt)
    # no list at all, and an empty table: no launch, zero gradients
    Ug = U.clone().requires_grad_(True)
    loss, lse, scores = evaluate.list_softmax(Ug[:0], R, I[:0], Cn[:0], Tt[:0])
    assert loss.shape == lse.shape == (0,) and scores.shape == (0, M)
    loss.sum().backward()
    assert (Ug.grad == 0).all()
    none = evaluate.list_softmax(U, R[:0], I, Cn, Tt)
    assert (none[0] == 0).all() and torch.isneginf(none[1]).all() and torch.isnan(none[2]).all()
    # users without a gradient, rows with one, and the other way round
    Rg = R.clone().requires_grad_(True)
    evaluate.list_softmax(U, Rg, I, Cn, Tt)[0].sum().backward()
    Ug = U.clone().requires_grad_(True)
    evaluate.list_softmax(Ug, R, I, Cn, Tt)[0].sum().backward()
    S = _gathered(users, rows, ids)
    w_dU, w_dR = evaluate.list_softmax_grad_host(users, rows, S, ids, count, teacher)
    close(Ug.grad, w_dU, "d_users alone", rtol=2e-4, atol=0.0)
    close(Rg.grad, w_dR, "d_rows alone", rtol=2e-4, atol=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# nrms.distil_step against the float64 CPU twin
# ---------------------------------------------------------------------------------------------------------------------
STEP_FIXTURE = "nrms_train_tiny.npz"      # test_hip_pool_softmax.py's: on the other fixtures stock fp32 itself misses 2e-4 on the pooling parameters


def _train_set(device="cpu"):
    dev = NC.dev_set(STEP_FIXTURE, device)
    U, K = NC.case(STEP_FIXTURE)[2]["candidate_ids"].shape
    dev.row_label = (np.arange(U * K) % K == 0).astype(np.int64)
    return dev, U


@functools.lru_cache(maxsize=None)
def _lists():
    """Per user a list of 12 news with repeats across users, a count below M, an id outside the corpus and a slot without mass."""
    dev, U = _train_set()
    N = int(dev.title_text.shape[0])
    rng = np.random.default_rng(17)
    M = 12
    ids = rng.integers(1, N, size=(U, M)).astype(np.int64)
    teacher = (1.5 * rng.standard_normal((U, M))).astype(np.float32)
    count = np.full(U, M, dtype=np.int32)
    count[1] = M - 3
    ids[0, 4], ids[2, 0] = N + 2, -1
    teacher[0, 1], teacher[3, :] = -np.inf, -np.inf
    teacher[3, 5] = 0.0
    return np.arange(U), ids, teacher, count


@functools.lru_cache(maxsize=None)
def _step_reference(pre):
    from digat_amd import nrms
    m = PC.double_twin(NC.model(STEP_FIXTURE, pre))
    m.train()
    dev, U = _train_set()
    loss = nrms.distil_step(m, dev, *_lists()[:3], _lists()[3], scale=1.0, temperature=2.0)
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy().copy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("pre", list(NC.MODELS))
def test_nrms_distil_step_on_the_device(pre):
    from digat_amd import nrms
    want_loss, want = _step_reference(pre)
    m = NC.model(STEP_FIXTURE, pre, _dev())
    m.train()
    dev, U = _train_set(_dev())
    loss = nrms.distil_step(m, dev, *_lists()[:3], _lists()[3], scale=1.0, temperature=2.0)
    loss.backward()
    print(pre, "distil loss", float(loss.detach()), "float64 twin", want_loss)
    close(loss, np.float64(want_loss), f"{pre} distil loss", rtol=2e-5, atol=1e-5)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad, want[k], f"{pre} grad {k}", rtol=2e-4, atol=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# util.score_lists on devset_tiny-sized data
# ---------------------------------------------------------------------------------------------------------------------
def _digat():
    from digat_amd import synthetic
    from digat_amd.model import Model, PrecomputedNewsEncoder
    kw, depth = synthetic.DEVSET_FIXTURES["devset_tiny"]
    spec = synthetic.SynthSpec(**kw)
    corpus = synthetic.make_corpus(spec)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, depth, seed=spec.seed + 1, bias_std=0.05)
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return spec, corpus, model.to(_dev()).eval()


def test_score_lists_holds_the_scores_recommend_returns_in_place():
    from digat_amd import util
    spec, corpus, model = _digat()
    dc = util.DeviceCorpus.from_numpy(corpus, _dev())
    rng = np.random.default_rng(3)
    N, G, M = spec.news_num, 6, 40
    users = rng.permutation(corpus.history.shape[0])[:G].astype(np.int64)
    ids = np.stack([rng.permutation(np.arange(1, N))[:M] for _ in range(G)]).astype(np.int64)
    count = np.array([M, 0, 17, M, 1, M + 5], dtype=np.int32)
    ids[0, 3], ids[3, 0], ids[3, M - 1] = -1, N, N + 7
    cnt = np.clip(count, 0, M)
    elem = (np.arange(M)[None, :] < cnt[:, None]) & (ids >= 0) & (ids < N)
    start = np.r_[0, np.cumsum(elem.sum(axis=1))].astype(np.int64)
    for max_rows in (util.RECOMMEND_MAX_ROWS, 45):
        got = util.score_lists(model, dc, users, ids, count, batch_size=256, max_rows=max_rows)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (G, M)
        got = got.cpu().numpy()
        assert np.isneginf(got[~elem]).all() and np.isfinite(got[elem]).all(), "-inf exactly where the slot is no element"
        r_ids, r_scores, r_count = (t.cpu().numpy() for t in util.recommend(model, dc, users, (ids[elem], start), M, exclude_history=False,
                                                                            batch_size=256, max_rows=max_rows))
        for g in range(G):
            assert int(r_count[g]) == int(elem[g].sum())
            by_id = dict(zip(r_ids[g, :r_count[g]].tolist(), _bits(r_scores[g, :r_count[g]]).tolist()))
            for j in np.flatnonzero(elem[g]):
                assert by_id[int(ids[g, j])] == int(_bits(got[g, j:j + 1])[0]), (max_rows, g, j)
