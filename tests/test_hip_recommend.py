"""GPU suite for top-k recommendation: ``digat_topk_segments`` against its numpy restatement (``evaluate.topk_segments_host``),
exactly, over every boundary the kernel has (wave, workgroup, chunk, multi-chunk merge); against the existing ranking kernel; its
outputs fully written; and ``util.recommend`` against the fp32 CPU oracle (oracle/digat_oracle.py), the reference-pinned
``devset_tiny`` fixture and ``compute_scores``' own ranks."""
import functools
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import digat_oracle as O

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5                 # the project's bound for pipeline scores against the oracle (test_hip_ablation_pipeline.py)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against topk_segments_host
# ---------------------------------------------------------------------------------------------------------------------
KINDS = ("normal", "four_levels", "all_equal", "zeros_and_infs", "nans")


def kind_scores(rng, kind, n):
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "four_levels":
        return (rng.integers(0, 4, size=n) * 0.25 - 0.5).astype(np.float32)
    if kind == "all_equal":
        return np.full(n, 0.375, dtype=np.float32)
    if kind == "zeros_and_infs":
        vals = np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -1.5], dtype=np.float32)
        return vals[rng.integers(0, len(vals), size=n)]
    x = rng.standard_normal(n).astype(np.float32)
    hole = rng.random(n) < 0.3
    x[hole] = np.nan
    x.view(np.uint32)[hole & (rng.random(n) < 0.5)] = 0xFFC00001           # negative NaNs with a payload among them
    return x


def ragged_batch(k, seed=0):
    """The lengths of the issue, kinds rotating over the segments so that the all-equal kind falls on 2 * CHUNK + 1 (its winners are
    exactly the first k positions, all in the first chunk of three) and zeros / infinities on 70 001; then the multi-chunk lengths
    once more under the kinds they have not met."""
    from digat_amd.evaluate import TOPK_CHUNK as CH
    rng = np.random.default_rng(seed)
    lengths = [0, 1, 2, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 1, 70001]
    kinds = [KINDS[(i + 2) % 5] for i in range(len(lengths))]
    assert kinds[15] == "all_equal" and kinds[16] == "zeros_and_infs"
    lengths += [CH + 1, 2 * CH + 1, 70001, 2 * CH + 1]
    kinds += ["nans", "four_levels", "normal", "nans"]
    start = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    scores = np.concatenate([kind_scores(rng, kd, n) for kd, n in zip(kinds, lengths)]).astype(np.float32)
    return scores, start


def assert_same(got, want, what):
    gs, gi, gc = (x.cpu().numpy() for x in got)
    ws, wi, wc = want
    assert gs.dtype == np.float32 and gi.dtype == np.int64 and gc.dtype == np.int32
    assert np.array_equal(gc, wc), (what, np.flatnonzero(gc != wc)[:8])
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert bad.size == 0, (what, "ids differ in segments", bad[:8], gi[bad[0]], wi[bad[0]])
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (what, "score bits differ")


@pytest.mark.parametrize("k", [1, 10, 32, 128])
def test_kernel_matches_the_host_selection_exactly(k):
    from digat_amd import evaluate
    scores, start = ragged_batch(k, seed=k)
    want = evaluate.topk_segments_host(scores, start, k)
    got = evaluate.topk_segments(_t(scores), _t(start), k)
    torch.cuda.synchronize()
    assert_same(got, want, f"k={k}")
    # the all-equal segment of 2 * CHUNK + 1: exactly the first k positions
    assert got[1][15].tolist() == list(range(k))


def skip_case(skip_len, k=10, seed=0):
    """Segments in four roles, cycling: the skip row holds the best element's id / leaves fewer than k elements / leaves none /
    holds nobody's id.  ids are random int64, half of them above 2^31; an id shared by many elements of a segment is how ONE skip
    entry removes many of them (repeated ids are distinct elements, skipped together)."""
    from digat_amd import evaluate
    from digat_amd.evaluate import TOPK_CHUNK as CH
    rng = np.random.default_rng(seed + skip_len)
    lengths = [0, 1, 5, 40, 300, 11, 12, 257, CH + 7, 3, 64, 40000, 2 * CH + 1, 700, 20000, 9]
    start = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    S = len(lengths)
    scores = np.concatenate([kind_scores(rng, KINDS[s % 5], n) for s, n in enumerate(lengths)]).astype(np.float32)
    ids = np.where(rng.random(len(scores)) < 0.5, rng.integers(0, 2 ** 31, size=len(scores)), rng.integers(2 ** 31, 2 ** 40, size=len(scores)))
    ids = ids.astype(np.int64)
    skip = rng.integers(2 ** 41, 2 ** 42, size=(S, skip_len)).astype(np.int64)            # ids nobody has
    roles = {"best": 0, "fewer": 0, "none": 0}
    for s, n in enumerate(lengths):
        a, b = int(start[s]), int(start[s + 1])
        slot = int(rng.integers(0, skip_len))
        if n == 0:
            continue
        if s % 4 == 0:
            best = evaluate.topk_segments_host(scores[a:b], np.array([0, n]), 1)[1][0, 0]
            skip[s, slot] = ids[a + best]
            roles["best"] += 1
        elif s % 4 == 1 and n > 3:
            shared = int(rng.integers(2 ** 33, 2 ** 34))
            keep = rng.choice(n, size=3, replace=False)                                    # three survivors, k = 10
            mask = np.ones(n, dtype=bool)
            mask[keep] = False
            ids[a:b][mask] = shared
            skip[s, slot] = shared
            roles["fewer"] += 1
        elif s % 4 == 2:
            ids[a:b] = 2 ** 35 + 5
            skip[s, slot] = 2 ** 35 + 5
            roles["none"] += 1
    assert all(roles.values()), roles
    return scores, start, ids, skip


@pytest.mark.parametrize("skip_len", [1, 50, 256])
def test_kernel_with_ids_and_skip_rows(skip_len):
    from digat_amd import evaluate
    k = 10
    scores, start, ids, skip = skip_case(skip_len, k)
    assert (ids > 2 ** 31).any() and (ids < 2 ** 31).any()
    want = evaluate.topk_segments_host(scores, start, k, ids=ids, skip=skip)
    assert (want[2] == 0).sum() >= 2 and ((want[2] > 0) & (want[2] < k)).any() and (want[2] == k).any()
    got = evaluate.topk_segments(_t(scores), _t(start), k, ids=_t(ids), skip=_t(skip))
    torch.cuda.synchronize()
    assert_same(got, want, f"skip_len={skip_len}")
    # ids without a skip row: the same call surface, nothing left out
    assert_same(evaluate.topk_segments(_t(scores), _t(start), k, ids=_t(ids)), evaluate.topk_segments_host(scores, start, k, ids=ids), "ids only")


def test_selection_agrees_with_the_ranking_kernel():
    """300 segments of lengths 1..300, quantised scores: the position returned in slot j has rank j + 1 under digat_rank_metrics."""
    from digat_amd import evaluate
    rng = np.random.default_rng(5)
    lengths = np.arange(1, 301)
    start = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    scores = (rng.integers(0, 6, size=int(start[-1])) * 0.5 - 1.0).astype(np.float32)
    row_seg = np.repeat(np.arange(300), lengths)
    sc = _t(scores)
    ranks, _ = evaluate.device_ranks_and_metrics(sc, row_seg)
    for k in (7, 128):
        _, pos, count = (x.cpu().numpy() for x in evaluate.topk_segments(sc, _t(start), k))
        assert np.array_equal(count, np.minimum(lengths, k))
        for s in range(300):
            m = int(count[s])
            assert np.array_equal(ranks[start[s] + pos[s, :m]], np.arange(1, m + 1)), (k, s)


def test_every_output_byte_is_written_whatever_the_workspace_holds():
    from digat_amd import _lib, evaluate
    k = 10
    scores, start, ids, skip = skip_case(50, k, seed=3)
    sc, st, idt, sk = _t(scores), _t(start), _t(ids), _t(skip)
    S, R = len(start) - 1, len(scores)
    L = _lib.lib()
    need = int(L.digat_topk_segments_workspace_bytes(R, S, k))
    runs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=_dev())
        out_s = torch.full((S, k), fill, dtype=torch.uint8, device=_dev()).repeat(1, 4).view(torch.float32)
        out_i = torch.full((S, k), fill, dtype=torch.uint8, device=_dev()).repeat(1, 8).view(torch.int64)
        out_c = torch.full((S,), fill, dtype=torch.uint8, device=_dev()).repeat(4).view(torch.int32)
        assert tuple(out_s.shape) == (S, k) and tuple(out_i.shape) == (S, k) and tuple(out_c.shape) == (S,)
        _lib.check(L.digat_topk_segments(sc.data_ptr(), st.data_ptr(), R, S, idt.data_ptr(), sk.data_ptr(), 50, k, out_s.data_ptr(),
                                         out_i.data_ptr(), out_c.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), "digat_topk_segments")
        torch.cuda.synchronize()
        runs.append((out_s.cpu().numpy(), out_i.cpu().numpy(), out_c.cpu().numpy()))
    (s1, i1, c1), (s0, i0, c0) = runs
    assert np.array_equal(c1, c0) and np.array_equal(i1, i0) and np.array_equal(s1.view(np.uint32), s0.view(np.uint32))
    beyond = np.arange(k)[None, :] >= c1[:, None]
    assert beyond.any() and (c1 == 0).any()
    assert np.all(np.isneginf(s1[beyond])) and np.all(i1[beyond] == -1)
    want = evaluate.topk_segments_host(scores, start, k, ids=ids, skip=skip)
    assert np.array_equal(c1, want[2]) and np.array_equal(i1, want[1]) and np.array_equal(s1.view(np.uint32), want[0].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# util.recommend on devset_tiny
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus():
    from digat_amd import synthetic
    kw, depth = synthetic.DEVSET_FIXTURES["devset_tiny"]
    spec = synthetic.SynthSpec(**kw)
    return spec, synthetic.make_corpus(spec), depth


def _state(name):
    from digat_amd import synthetic
    spec, _, depth = _corpus()
    if name == "DIGAT":
        return synthetic.make_state_dict(spec.embedding_dim, spec.category_num, depth, seed=spec.seed + 1, bias_std=0.05)
    return synthetic.make_ablation_state_dict(name, spec.embedding_dim, spec.category_num, depth, seed=spec.seed + 1, bias_std=0.05)


def _model(name):
    from digat_amd.model import Model, PrecomputedNewsEncoder
    spec, corpus, depth = _corpus()
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder=name, news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in _state(name).items()}, strict=True)
    return model.to(_dev()).eval()


def _users():
    """Six impressions of the corpus, the fourth with an empty history."""
    _, corpus, _ = _corpus()
    length = corpus.extra["history_len"]
    empty, full = np.flatnonzero(length == 0), np.flatnonzero(length >= 3)
    users = np.array([full[0], full[1], full[2], empty[0], full[3], full[-1]], dtype=np.int64)
    assert not corpus.history[users[3]].any()
    return users


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """fp32 CPU oracle scores [6, news_num] of every (user, news) pair of ``_users()`` (column 0, the PAD news, included)."""
    spec, corpus, depth = _corpus()
    users = torch.from_numpy(_users())
    p = O.as_params(_state(name))
    emb = torch.from_numpy(corpus.news_embedding)
    Xn = emb[torch.from_numpy(corpus.news_node_ID.astype(np.int64))]
    An, Mn = torch.from_numpy(corpus.news_graph), torch.from_numpy(corpus.news_graph_mask)
    hist = torch.from_numpy(corpus.history.astype(np.int64))
    Au, cm = torch.from_numpy(corpus.user_graph), torch.from_numpy(corpus.user_category_mask)
    ci = torch.from_numpy(corpus.user_category_indices)
    P = spec.news_num
    out = []
    with torch.no_grad():
        c0 = O.news_graph_context(p, Xn, Mn)
        for u in users:
            rep = u.repeat(P)
            ue, au, cmu, ciu = emb[hist[rep]], Au[rep], cm[rep], ci[rep]
            if name == "DIGAT":
                out.append(O.row_logits(p, depth, ue, au, cmu, ciu, Xn, An, Mn, c0))
            else:
                n, v = O.ablation_encode(name, p, depth, Xn, An, Mn, ue, au, cmu, ciu, c_n=c0)
                out.append((n * v).sum(dim=1))
    res = torch.stack(out).numpy()
    res.setflags(write=False)
    return res


def check_against_oracle(name, ids, scores, count, k, exclude_history, what=""):
    """Scores by id within the bound; the returned set a valid top-k under the oracle up to twice the bound; scores non-increasing;
    no id twice; the exclusion honoured."""
    spec, corpus, _ = _corpus()
    ref = _oracle(name)
    users = _users()
    ids, scores, count = ids.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy()
    assert ids.shape == scores.shape == (len(users), k) and count.shape == (len(users),)
    for g, u in enumerate(users):
        eligible = np.ones(spec.news_num, dtype=bool)
        eligible[0] = False                                       # the pool is every non-PAD news
        if exclude_history:
            eligible[corpus.history[u]] = False
        m = int(count[g])
        assert m == min(k, int(eligible.sum())), (what, g)
        got_ids, got = ids[g, :m], scores[g, :m]
        assert len(set(got_ids.tolist())) == m and eligible[got_ids].all(), (what, g, got_ids)
        if exclude_history:
            assert 0 not in got_ids and not np.isin(got_ids, corpus.history[u]).any()
        assert np.all(np.diff(got) <= 0), (what, g, got)
        want = ref[g, got_ids]
        err = np.abs(got - want)
        print(f"[{name} {what} user {g}] max|d| {err.max():.3e} at |ref| {np.abs(want).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=f"{what} user {g}")
        kth = np.sort(ref[g][eligible])[::-1][m - 1]
        slack = 2 * (ATOL + RTOL * abs(float(kth)))
        assert (want >= kth - slack).all(), (what, g, "a returned news lies below the oracle's k-th best", float((kth - want).max()))
        left_out = eligible.copy()
        left_out[got_ids] = False
        assert (ref[g][left_out] <= kth + slack).all(), (what, g, "a news left out lies above the oracle's k-th best")


def _pool():
    spec, _, _ = _corpus()
    return np.arange(1, spec.news_num, dtype=np.int64)


@pytest.mark.parametrize("name", ["DIGAT", "wo_interaction"])
def test_recommend_against_the_oracle(name):
    from digat_amd import util
    _, corpus, _ = _corpus()
    model = _model(name)
    dc = util.DeviceCorpus.from_numpy(corpus, _dev())
    k = 10
    for exclude in (True, False):
        ids, scores, count = util.recommend(model, dc, _users(), _pool(), k, exclude_history=exclude, batch_size=256)
        assert ids.is_cuda and ids.dtype == torch.int64 and scores.dtype == torch.float32 and count.dtype == torch.int32
        check_against_oracle(name, ids, scores, count, k, exclude, what=f"exclude={exclude}")


@pytest.mark.parametrize("user_graphs", ["table", "derived"])
def test_users_as_indices_and_as_arrays_agree_bit_for_bit(user_graphs):
    from digat_amd import util
    _, corpus, _ = _corpus()
    model = _model("DIGAT")
    dc = util.DeviceCorpus.from_numpy(corpus, _dev(), user_graphs=user_graphs)
    users = _users()
    by_index = util.recommend(model, dc, users, _pool(), 10, batch_size=256)
    arrays = (corpus.history[users].astype(np.int64), corpus.user_category_indices[users])
    by_array = util.recommend(model, dc, arrays, _pool(), 10, batch_size=256)
    assert torch.equal(by_index[0], by_array[0]) and torch.equal(by_index[2], by_array[2])
    assert torch.equal(by_index[1].view(torch.int32), by_array[1].view(torch.int32))
    check_against_oracle("DIGAT", *by_array, 10, True, what=user_graphs)


def test_recommend_over_each_impressions_own_candidates():
    """Every impression's own candidate list (CSR), k = 5, nothing excluded: the reference's scores of the same rows
    (tests/golden/devset_tiny.npz) within test_hip_parity.py's tolerance for that fixture, the set a valid top-5 under them, and the
    ids in the order of ``compute_scores``' ranks."""
    from digat_amd import evaluate, util
    _, corpus, _ = _corpus()
    fx = load_golden("devset_tiny.npz")
    rtol, atol = 1e-4, 2e-4
    model = _model("DIGAT")
    dc = util.DeviceCorpus.from_numpy(corpus, _dev())
    I = corpus.history.shape[0]
    imp = corpus.row_impression
    start = np.r_[0, np.cumsum(np.bincount(imp, minlength=I))].astype(np.int64)
    k = 5
    ids, scores, count = (x.cpu().numpy() for x in util.recommend(model, dc, np.arange(I), (corpus.row_candidate.astype(np.int64), start), k,
                                                                  exclude_history=False, batch_size=256))
    own, _ = util.compute_scores(model, dc, 256)
    ranks = evaluate.impression_ranks(own, imp)
    ref = fx["scores"]
    for i in range(I):
        a, b = int(start[i]), int(start[i + 1])
        m = int(count[i])
        assert m == min(k, b - a)
        cand = corpus.row_candidate[a:b].astype(np.int64)
        order = np.argsort(ranks[a:b], kind="stable")[:m]
        assert np.array_equal(ids[i, :m], cand[order]), i
        assert np.all(np.diff(scores[i, :m]) <= 0)
        first = {int(c): j for j, c in reversed(list(enumerate(cand)))}             # a candidate listed twice scores the same
        rows = np.array([first[int(c)] for c in ids[i, :m]])
        want = ref[a:b][rows]
        np.testing.assert_allclose(scores[i, :m], want, rtol=rtol, atol=atol, err_msg=str(i))
        kth = np.sort(ref[a:b])[::-1][m - 1]
        slack = 2 * (atol + rtol * abs(float(kth)))
        assert (want >= kth - slack).all(), i
        rest = np.ones(b - a, dtype=bool)
        rest[order] = False
        assert (ref[a:b][rest] <= kth + slack).all(), i


def test_three_user_chunks_match_one():
    from digat_amd import util
    spec, corpus, _ = _corpus()
    model = _model("DIGAT")
    dc = util.DeviceCorpus.from_numpy(corpus, _dev())
    k, P = 10, spec.news_num - 1
    assert util.recommend_user_chunks(6, P, None, 2 * P) == [(0, 2), (2, 4), (4, 6)]
    one = util.recommend(model, dc, _users(), _pool(), k, batch_size=256)
    three = util.recommend(model, dc, _users(), _pool(), k, batch_size=256, max_rows=2 * P)
    check_against_oracle("DIGAT", *one, k, True, what="one chunk")
    check_against_oracle("DIGAT", *three, k, True, what="three chunks")
    ids1, s1 = one[0].cpu().numpy(), one[1].cpu().numpy()
    ids3, s3 = three[0].cpu().numpy(), three[1].cpu().numpy()
    for g in range(6):
        by_id = dict(zip(ids1[g].tolist(), s1[g].tolist()))
        common = [i for i in ids3[g].tolist() if i in by_id]
        assert common, g
        np.testing.assert_allclose([dict(zip(ids3[g].tolist(), s3[g].tolist()))[i] for i in common], [by_id[i] for i in common],
                                   rtol=RTOL, atol=ATOL)
