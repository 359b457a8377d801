"""No GPU: the numpy twin of the pairwise nDCG loss (``evaluate.list_pairwise_host`` / ``_grad_host``) against an independent float64
autograd loop; ``evaluate.list_pairwise`` and ``pairwise_scores`` on CPU float64 tensors against the twin; its ``ndcg`` against the
nDCG@5 / nDCG@10 the evaluation prints; the closed form of one pair; the discount table; refusals; ``nrms.rank_step``, ``fit_ranker``
and ``impression_gain_lists`` on CPU tensors."""
import math

import numpy as np
import pytest
import torch

import list_pairwise_common as LP
import nrms_common as NC
import pool_softmax_common as PC

FIXTURE = "nrms_train_tiny.npz"


def _dyadic_case(rng, G, M, d, shift=0):
    """``LP.case`` with vectors on a grid of 1/8: every inner product is a multiple of 1/64 below 2^10, exact in float32 and in
    float64 alike, so the float64 composition and the twin (which rounds ``scale * score`` to float32) see the same x."""
    users, rows, ids, count, gain, kind = LP.case(rng, G, M, d, shift)
    users = (rng.integers(-8, 9, size=users.shape) / 8.0).astype(np.float32)
    rows = (rng.integers(-8, 9, size=rows.shape) / 8.0).astype(np.float32)
    return users, rows, ids, count, gain, kind


def _scores(users, rows, ids):
    ok = (ids >= 0) & (ids < len(rows))
    S = users.astype(np.float64) @ rows.astype(np.float64).T
    return np.where(ok, S[np.arange(len(ids))[:, None], np.where(ok, ids, 0)], 0.0).astype(np.float32)


def _close(got, want, what, rtol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    size = np.abs(want).max() if want.size else 0.0
    err = np.abs(got - want).max() if want.size else 0.0
    assert err <= rtol * max(size, 1e-300) or err == 0, (what, err, size)


def test_ndcg_discount_values_and_truncation():
    from digat_amd import evaluate
    D = evaluate.ndcg_discount(12)
    assert D.dtype == np.float64 and D.shape == (12,) and D[0] == 1.0
    assert np.array_equal(D, 1.0 / np.log2(2.0 + np.arange(12)))
    assert abs(D[1] - 1.0 / math.log2(3.0)) <= 1e-16 and D[2] == 0.5 and (np.diff(D) < 0).all()
    D5 = evaluate.ndcg_discount(12, 5)
    assert np.array_equal(D5[:5], D[:5]) and (D5[5:] == 0).all()
    assert np.array_equal(evaluate.ndcg_discount(3, 5), D[:3]) and evaluate.ndcg_discount(0).shape == (0,)
    with pytest.raises(ValueError):
        evaluate.ndcg_discount(-1)


@pytest.mark.parametrize("k", [0, 5])
def test_the_twin_against_the_independent_autograd_loop(k):
    from digat_amd import evaluate
    rng = np.random.default_rng(11 + k)
    seen = set()
    for G, M, d, scale in ((7, 37, 6, 1.0), (12, 20, 3, 0.5), (6, 1, 2, 1.0), (6, 2, 2, 1.0)):
        users, rows, ids, count, gain, kind = LP.case(rng, G, M, d, shift=k)
        seen |= set(kind.tolist())
        S = _scores(users, rows, ids)
        D = evaluate.ndcg_discount(M, k)
        for cnt in (count, None):
            want = LP.stock_fp64(S, ids, cnt, gain, len(rows), scale, D)
            got = evaluate.list_pairwise_host(S, ids, cnt, gain, len(rows), scale, D)
            assert np.array_equal(got[2], want[2]), "valid"
            for a, b, name in zip(got, want, ("loss", "ndcg", "valid", "lambda")):
                _close(a, b, (G, M, name))
            assert (got[0][~want[2]] == 0).all() and (got[1][~want[2]] == 0).all() and (got[3][~want[2]] == 0).all()
            single = (kind == LP.KINDS.index("single")) & want[2]
            assert (got[0][single] == 0).all() and (got[1][single] == 1).all(), "one labelled element: no pair, ndcg 1"
        # given scores: NaN marks what is no element
        Sn = np.where(LP.elements(ids, None, len(rows)), S, np.float32(np.nan))
        want = LP.stock_fp64(Sn, None, count, gain, 0, scale, D)
        got = evaluate.list_pairwise_host(Sn, None, count, gain, 0, scale, D)
        same = evaluate.list_pairwise_host(S, ids, count, gain, len(rows), scale, D)
        for a, b, c, name in zip(got, want, same, ("loss", "ndcg", "valid", "lambda")):
            _close(a, b, (G, M, name, "scores"))
            assert np.array_equal(a, c), "the scores contract on NaN-marked scores is the ids contract"
    assert seen == set(range(len(LP.KINDS))), "every kind of gains occurs"


def test_the_unlabelled_take_part_in_nothing():
    from digat_amd import evaluate
    rng = np.random.default_rng(3)
    users, rows, ids, count, gain, kind = LP.case(rng, 6, 30, 4, shift=5)      # list 0: NaN, -inf, +inf and a negative gain
    count[:] = 30
    S = _scores(users, rows, ids)
    full = evaluate.list_pairwise_host(S, ids, count, gain, len(rows))
    with np.errstate(invalid="ignore"):
        off = ~(np.isfinite(gain[0]) & (gain[0] >= 0))
    assert off.sum() == 4 and (full[3][0][off] == 0).all()
    keep = np.flatnonzero(~off)
    alone = evaluate.list_pairwise_host(S[:1, keep], ids[:1, keep], None, gain[:1, keep], len(rows), discount=evaluate.ndcg_discount(30)[:len(keep)])
    assert alone[0][0] == full[0][0] and alone[1][0] == full[1][0] and np.array_equal(alone[3][0], full[3][0][keep])


@pytest.mark.parametrize("k", [0, 5])
def test_the_cpu_composition_against_the_twin(k):
    from digat_amd import evaluate
    rng = np.random.default_rng(5 + k)
    for G, M, d, scale in ((8, 33, 5, 0.5), (6, 9, 3, 2.0)):
        users, rows, ids, count, gain, kind = _dyadic_case(rng, G, M, d, shift=k)
        P = len(rows)
        D = evaluate.ndcg_discount(M, k)
        S = _scores(users, rows, ids)
        assert np.array_equal(S.astype(np.float64), np.where((ids >= 0) & (ids < P), (users.astype(np.float64) @ rows.astype(np.float64).T)[
            np.arange(G)[:, None], np.clip(ids, 0, P - 1)], 0.0)), "the grid keeps the products exact"
        gl = rng.standard_normal(G)
        w_loss, w_ndcg, w_valid, w_lam = evaluate.list_pairwise_host(S, ids, count, gain, P, scale, D)
        w_dU, w_dR = evaluate.list_pairwise_grad_host(users, rows, S, ids, count, gain, scale, D, gl)
        U = torch.tensor(users, dtype=torch.float64, requires_grad=True)
        R = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
        loss, ndcg, scores = evaluate.list_pairwise(U, R, torch.from_numpy(ids), torch.from_numpy(count), torch.from_numpy(gain), scale=scale,
                                                    discount=D)
        assert loss.requires_grad and not ndcg.requires_grad and not scores.requires_grad and loss.dtype == torch.float64
        (loss * torch.from_numpy(gl)).sum().backward()
        elem = LP.elements(ids, count, P)
        assert np.array_equal(np.isnan(scores.numpy()), ~elem) and np.array_equal(scores.numpy()[elem], S[elem].astype(np.float64))
        _close(loss.detach().numpy(), w_loss, "loss")
        _close(ndcg.numpy(), w_ndcg, "ndcg")
        _close(U.grad.numpy(), w_dU, "d_users")
        _close(R.grad.numpy(), w_dR, "d_rows")
        assert (loss.detach().numpy()[~w_valid] == 0).all() and (U.grad.numpy()[~w_valid] == 0).all()
        # the same loss on given scores; its gradient is grad_loss lambda
        Sn = np.where(elem, S.astype(np.float64), np.nan)
        St = torch.tensor(Sn, requires_grad=True)
        for cnt in (torch.from_numpy(count), None):
            St.grad = None
            p_loss, p_ndcg = evaluate.pairwise_scores(St, cnt, torch.from_numpy(gain), scale=scale, discount=D)
            (p_loss * torch.from_numpy(gl)).sum().backward()
            _close(p_loss.detach().numpy(), w_loss, "scores loss")
            _close(p_ndcg.numpy(), w_ndcg, "scores ndcg")
            _close(St.grad.numpy(), gl[:, None] * w_lam, "scores gradient")
            assert (St.grad.numpy()[w_lam == 0] == 0).all()


def test_ndcg_is_the_ndcg_the_evaluation_prints():
    from digat_amd import evaluate
    rng = np.random.default_rng(8)
    sizes = [2, 3, 7, 12, 12, 25, 5, 40]
    M = max(sizes)
    labels, scores, imp = [], [], []
    for i, n in enumerate(sizes):
        y = np.zeros(n, dtype=np.int64)
        y[rng.choice(n, size=int(rng.integers(1, max(2, n // 3))), replace=False)] = 1      # a positive and a negative in every impression
        assert 0 < y.sum() < n
        labels.append(y)
        scores.append(rng.integers(-6, 7, size=n) * 0.25)                                   # many ties
        imp.append(np.full(n, i))
    labels, scores, imp = np.concatenate(labels), np.concatenate(scores), np.concatenate(imp)
    assert any(len(np.unique(scores[imp == i])) < n for i, n in enumerate(sizes))
    rows = evaluate.impression_metric_rows(labels, evaluate.impression_ranks(scores, imp), imp)
    S = np.full((len(sizes), M), np.nan, dtype=np.float32)
    gain = np.full((len(sizes), M), np.nan, dtype=np.float32)
    for i, n in enumerate(sizes):
        S[i, :n], gain[i, :n] = scores[imp == i], labels[imp == i]
    count = np.array(sizes, dtype=np.int32)
    for k, col in ((5, 2), (10, 3)):
        D = evaluate.ndcg_discount(M, k)
        ndcg = evaluate.list_pairwise_host(S, None, count, gain, 0, 1.0, D)[1]
        assert np.abs(ndcg - rows[:, col]).max() <= 4 * np.finfo(np.float64).eps, (k, np.abs(ndcg - rows[:, col]).max())
        t_ndcg = evaluate.pairwise_scores(torch.from_numpy(S).double(), torch.from_numpy(count), torch.from_numpy(gain), discount=D)[1].numpy()
        assert np.abs(t_ndcg - rows[:, col]).max() <= 4 * np.finfo(np.float64).eps


def test_one_pair_in_closed_form():
    from digat_amd import evaluate
    D = evaluate.ndcg_discount(2)
    for x0, x1 in ((0.5, -1.25), (-2.0, 3.0), (1.0, 1.0), (300.0, -300.0), (-300.0, 300.0)):
        S = np.array([[x0, x1]], dtype=np.float32)
        gain = np.array([[1.0, 0.0]], dtype=np.float32)
        loss, ndcg, valid, lam = evaluate.list_pairwise_host(S, None, None, gain, 0, 1.0, D)
        t = x0 - x1
        want = (D[0] - D[1]) * (max(-t, 0.0) + math.log1p(math.exp(-abs(t))))      # idcg = 1
        assert valid[0] and abs(loss[0] - want) <= 1e-15 * want, (x0, x1)
        assert ndcg[0] == (1.0 if x0 >= x1 else D[1])
        assert lam[0, 0] == -lam[0, 1] and lam[0, 0] <= 0 and np.isfinite(lam).all()
        t_loss = evaluate.pairwise_scores(torch.from_numpy(S).double(), None, torch.from_numpy(gain))[0]
        assert abs(float(t_loss[0]) - want) <= 1e-15 * want


def test_refusals():
    from digat_amd import evaluate
    rng = np.random.default_rng(1)
    users, rows, ids, count, gain, _ = LP.case(rng, 4, 9, 3)
    U, R, I, Cn, Gn = (torch.from_numpy(x) for x in (users, rows, ids, count, gain))
    D = evaluate.ndcg_discount(9)
    up = D.copy()
    up[3] = up[2] * 1.5
    neg = D.copy()
    neg[-1] = -0.1
    inf = D.copy()
    inf[0] = np.inf
    for bad, word in ((D.astype(np.float32), "float64"), (up, "non-increasing"), (neg, "non-negative"), (inf, "finite"), (D[:8], "one value per rank"),
                      (D[None], "one value per rank")):
        with pytest.raises(ValueError, match=word):
            evaluate.list_pairwise(U, R, I, Cn, Gn, discount=bad)
        with pytest.raises(ValueError, match=word):
            evaluate.pairwise_scores(torch.zeros(4, 9), Cn, Gn, discount=bad)
        with pytest.raises(ValueError, match=word):
            evaluate.list_pairwise_host(np.zeros((4, 9), dtype=np.float32), ids, count, gain, len(rows), 1.0, bad)
    evaluate.list_pairwise(U, R, I, Cn, Gn, discount=1.0 / (1.0 + np.arange(9.0)))          # any non-increasing table
    with pytest.raises(ValueError, match="share d"):
        evaluate.list_pairwise(U, R[:, :2], I, Cn, Gn)
    with pytest.raises(ValueError, match="ids must be"):
        evaluate.list_pairwise(U, R, I[:2], Cn, Gn)
    with pytest.raises(ValueError, match="gain must be"):
        evaluate.list_pairwise(U, R, I, Cn, Gn[:, :3])
    with pytest.raises(ValueError, match="gain must be"):
        evaluate.list_pairwise(U, R, I, Cn, Gn.long())
    with pytest.raises(ValueError, match="count must be"):
        evaluate.list_pairwise(U, R, I, Cn[:2], Gn)
    with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
        evaluate.list_pairwise(U, R, torch.zeros(4, 1025, dtype=torch.int64), Cn, torch.zeros(4, 1025))
    with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
        evaluate.pairwise_scores(torch.zeros(4, 1025), None, torch.zeros(4, 1025))
    with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
        evaluate.list_pairwise(U, R, I[:, :0], Cn, Gn[:, :0])
    with pytest.raises(ValueError, match="LIST_SOFTMAX_MAX_D"):
        evaluate.list_pairwise(torch.zeros(4, 513), torch.zeros(5, 513), I, Cn, Gn)
    with pytest.raises(ValueError, match="scores must be"):
        evaluate.pairwise_scores(torch.zeros(4, 9, dtype=torch.int64), Cn, Gn)


# ---------------------------------------------------------------------------------------------------------------------
# nrms.rank_step, fit_ranker, impression_gain_lists on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def _train_set():
    dev = NC.dev_set(FIXTURE, "cpu")
    U, K = NC.case(FIXTURE)[2]["candidate_ids"].shape
    dev.row_label = (np.arange(U * K) % K == 0).astype(np.int64)
    return dev, U, K


def test_impression_gain_lists_against_a_python_loop():
    from digat_amd import nrms
    dev, U, K = _train_set()
    dev.row_impression = np.array([0, 0, 0, 2, 2, 1, 3, 3, 3, 3])
    dev.row_candidate = np.array([5, 6, 7, 8, 9, 4, 1, 2, 3, 1])
    dev.row_label = np.array([0, 1, 1, 0, 0, 1, 0, 0, 0, 1])
    users, ids, gain, count = nrms.impression_gain_lists(dev)
    t_users, t_ids, t_teacher, t_count = nrms.impression_lists(dev)
    assert np.array_equal(users, t_users) and np.array_equal(ids, t_ids) and np.array_equal(count, t_count)
    assert gain.dtype == np.float32 and count.dtype == np.int32
    want = np.full(ids.shape, np.nan)
    for u, i in enumerate(users):
        at = [r for r in range(len(dev.row_impression)) if dev.row_impression[r] == i]
        for j, r in enumerate(at):
            assert ids[u, j] == dev.row_candidate[r]
            want[u, j] = 1.0 if dev.row_label[r] == 1 else 0.0
    assert np.array_equal(gain, want, equal_nan=True)
    assert gain.tolist()[0][:3] == [0.0, 1.0, 1.0] and np.isnan(gain[0, 3]) and np.isnan(gain[1, 1:]).all()
    only = nrms.impression_gain_lists(dev, users=np.array([2]))
    assert only[2].tolist() == [[0.0, 0.0]]


@pytest.mark.parametrize("pre", list(NC.MODELS))
def test_rank_step_is_the_mean_of_the_valid_lists(pre):
    from digat_amd import evaluate, nrms
    dev, U, K = _train_set()
    m = PC.double_twin(NC.model(FIXTURE, pre)).eval()
    lists = nrms.impression_gain_lists(dev)
    g = 2
    loss = nrms.rank_step(m, dev, lists[0][g:g + 1], lists[1][g:g + 1], lists[2][g:g + 1], lists[3][g:g + 1], k=5)
    cand = torch.from_numpy(lists[1][g])
    sa = pre == "sa"
    with torch.no_grad():
        news = m.news_encoder.forward_stock(dev.title_text[cand][None], dev.title_mask[cand][None],
                                            dev.augmented_title_text[cand][None] if sa else None,
                                            dev.augmented_title_mask[cand][None] if sa else None)[0]
        hist = dev.history_ids[g:g + 1].to(torch.int64)
        user = m.user_encoder.forward_stock(dev.title_text[hist], dev.title_mask[hist], dev.history_mask[g:g + 1])[0]
        x = (news @ user).numpy()
    # one click at slot 0 against K - 1 negatives, from the definition
    D = evaluate.ndcg_discount(K, 5)
    rank = [sum(1 for b in range(K) if x[b] > x[a] or (x[b] == x[a] and b < a)) for a in range(K)]
    want = sum(abs(D[rank[0]] - D[rank[b]]) / D[0] * (max(-(x[0] - x[b]), 0.0) + math.log1p(math.exp(-abs(x[0] - x[b])))) for b in range(1, K))
    assert loss.requires_grad and abs(float(loss.detach()) - want) <= 1e-10 * abs(want)
    gain, count = lists[2].copy(), lists[3].copy()
    gain[1] = 0.0                                                   # no positive gain: invalid
    count[3] = 0
    all_ = nrms.rank_step(m, dev, lists[0], lists[1], gain, count)
    each = [float(nrms.rank_step(m, dev, lists[0][i:i + 1], lists[1][i:i + 1], gain[i:i + 1], count[i:i + 1]).detach()) for i in range(U)]
    assert each[1] == 0 and each[3] == 0 and abs(float(all_.detach()) - sum(each) / (U - 2)) <= 1e-10 * abs(float(all_.detach()))
    nothing = nrms.rank_step(m, dev, lists[0][:2], lists[1][:2], gain[:2], np.zeros(2, dtype=np.int32))
    assert float(nothing.detach()) == 0
    nothing.backward()
    with pytest.raises(ValueError, match="must be a floating-point array"):
        nrms.rank_step(m, dev, lists[0], lists[1], gain[:, :2], count)


def _mean_ndcg(m, dev, lists):
    from digat_amd import evaluate, nrms
    m.eval()
    with torch.no_grad():
        idx, ids, gain, count = nrms._check_lists(*lists[:3], lists[3], int(dev.history_ids.shape[0]))
        user, table, pos, cnt, _ = nrms._list_front(m, dev, idx, ids, count)
        return float(evaluate.list_pairwise(user, table, pos, cnt, torch.from_numpy(gain).to(user.dtype))[1].mean())


def test_fit_ranker_is_seeded_and_raises_the_ndcg_of_its_lists():
    """A direction check with no threshold: float64 CPU copy, fixed seed — the mean nDCG of the fixed lists in eval mode is higher
    after the steps than before; two runs with the same draws give identical losses."""
    from digat_amd import nrms
    dev, U, K = _train_set()
    lists = nrms.impression_gain_lists(dev)
    m = PC.double_twin(NC.model(FIXTURE, "nrms"))
    before = _mean_ndcg(m, dev, lists)
    losses = nrms.fit_ranker(m, dev, lists, 8, batch_users=3, lr=1e-3, seed=5)
    after = _mean_ndcg(m, dev, lists)
    print("mean nDCG before", before, "after", after, "step losses", losses)
    assert len(losses) == 8 and all(np.isfinite(losses)) and after > before
    again = PC.double_twin(NC.model(FIXTURE, "nrms"))
    assert nrms.fit_ranker(again, dev, lists, 2, batch_users=3, lr=1e-3, seed=5) == losses[:2], "seeded draws"
    with pytest.raises(ValueError, match="lists must be"):
        nrms.fit_ranker(m, dev, lists[:3], 1)
    with pytest.raises(ValueError, match="no list"):
        nrms.fit_ranker(m, dev, (lists[0][:0], lists[1][:0], lists[2][:0], lists[3][:0]), 1)
