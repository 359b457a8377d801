"""GPU suite: long shortlists — ``digat_shortlist_segments`` and ``digat_dot_shortlist`` held exactly (score bits, ids, counts) to the
host contracts ``evaluate.shortlist_segments_host`` / ``dot_shortlist_host``, to the 128-entry selections they extend and to
``dot_rank``; their behaviour on malformed offsets, a poisoned workspace and a side stream; ``nrms.shortlist`` on the device and into
the re-rank.  Everything is a selection of stored bits: no tolerance anywhere."""
import functools
import types

import numpy as np
import pytest
import torch

import dot_topk_common as D
import shortlist_common as SC

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.array(x)).to(_dev())             # a copy: the cached cases are read-only


def _host(t):
    return tuple(x.cpu().numpy() for x in t)


VARIANTS = ((False, 0), (True, 0), (True, 50), (True, 256))      # (ids, skip entries)


@functools.lru_cache(maxsize=None)
def _cases(m):
    """Every kind of values under every (ids, skip) variant for list length m, with the host contract's answer: computed once."""
    from digat_amd import evaluate
    rng = np.random.default_rng(100 + m)
    out = []
    for kind in SC.KINDS:
        for with_ids, skip_len in VARIANTS:
            x, start, ids, skip = SC.segment_case(rng, m, kind, with_ids, skip_len)
            want = evaluate.shortlist_segments_host(x, start, m, ids=ids, skip=skip)
            for a in (x, start, ids, skip) + want:
                if a is not None:
                    a.setflags(write=False)
            out.append(((kind, with_ids, skip_len), x, start, ids, skip, want))
    return out


@pytest.mark.parametrize("m", SC.MS)
def test_segments_equal_the_host_contract(m):
    from digat_amd import evaluate
    for what, x, start, ids, skip, want in _cases(m):
        got = evaluate.shortlist_segments(_t(x), _t(start), m, ids=_t(ids), skip=_t(skip))
        SC.same(got, want, (m,) + what)
        lens = np.diff(start)
        if skip is None:
            assert np.array_equal(want[2], np.minimum(lens, m))
        else:
            assert (want[2] < np.minimum(lens, m)).any(), "a skip row removes elements"


@pytest.mark.parametrize("m", SC.MS)
def test_segments_extend_topk_segments(m):
    """Up to 128 entries the outputs are topk_segments', bit for bit; of a longer list the first 128 columns are topk_segments(128)'s."""
    from digat_amd import evaluate
    k = min(m, evaluate.TOPK_MAX_K)
    for what, x, start, ids, skip, _ in _cases(m):
        X, ST, I, SK = _t(x), _t(start), _t(ids), _t(skip)
        s, i, c = _host(evaluate.shortlist_segments(X, ST, m, ids=I, skip=SK))
        SC.same((s[:, :k], i[:, :k], np.minimum(c, k)), evaluate.topk_segments(X, ST, k, ids=I, skip=SK), (m,) + what)


def _guarded(n, dtype, fill):
    """A buffer of n elements inside a larger one holding ``fill``: (whole, view)."""
    pad = 4096
    whole = torch.full((n + 2 * pad,), fill, dtype=dtype, device=_dev())
    return whole, whole[pad:pad + n]


def _guards_intact(whole, n, fill):
    pad = 4096
    return bool((whole[:pad] == fill).all()) and bool((whole[pad + n:] == fill).all())


def test_malformed_offsets_stay_inside_the_arrays_and_every_output_byte_is_written():
    from digat_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(9)
    R, m = 3 * SC.CHUNK + 77, 300
    x = rng.standard_normal(R).astype(np.float32)
    ids = rng.integers(0, 5000, size=R).astype(np.int64)
    starts = {
        "decreasing": [0, 2 * SC.CHUNK + 9, SC.CHUNK, 500, R, 40],
        "overshooting": [-7, 5, R + 1000, R + 5, 1 << 40, R],
        "negative": [-(1 << 40), -5, -1, 3, 2000, SC.CHUNK + 5],
        "zigzag": [R + 9, 0, 3 * SC.CHUNK, 5, R, 0],
        "well formed": [0, 0, 700, 700 + SC.CHUNK, R - 1, R],
    }
    S = 5
    need = int(L.digat_shortlist_segments_workspace_bytes(R, S, m))
    X, I = _t(x), _t(ids)
    skip = _t(rng.integers(0, 5000, size=(S, 50)).astype(np.int64))
    SCORE_FILL, ID_FILL, COUNT_FILL = 123.0, 0x5555555555555555, 0x55555555
    for name, st in starts.items():
        ws_whole, ws = _guarded(need, torch.uint8, 0xA5)
        s_whole, out_s = _guarded(S * m, torch.float32, SCORE_FILL)
        i_whole, out_i = _guarded(S * m, torch.int64, ID_FILL)
        c_whole, out_c = _guarded(S, torch.int32, COUNT_FILL)
        assert ws.data_ptr() % 8 == 0
        ST = _t(np.array(st, dtype=np.int64))
        _lib.check(L.digat_shortlist_segments(X.data_ptr(), ST.data_ptr(), R, S, I.data_ptr(), skip.data_ptr(), 50, m, out_s.data_ptr(),
                                              out_i.data_ptr(), out_c.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), name)
        torch.cuda.synchronize()
        assert _guards_intact(ws_whole, need, 0xA5) and _guards_intact(s_whole, S * m, SCORE_FILL), name
        assert _guards_intact(i_whole, S * m, ID_FILL) and _guards_intact(c_whole, S, COUNT_FILL), name
        s, i, c = out_s.view(S, m).cpu().numpy(), out_i.view(S, m).cpu().numpy(), out_c.cpu().numpy()
        assert (i != ID_FILL).all() and (c != COUNT_FILL).all() and (s != SCORE_FILL).all(), (name, "an output byte was not written")
        assert ((0 <= c) & (c <= m)).all(), name
        for g in range(S):
            assert (i[g, c[g]:] == -1).all() and np.isneginf(s[g, c[g]:]).all(), name
            assert ((0 <= i[g, :c[g]]) & (i[g, :c[g]] < 5000)).all(), name
        if name == "well formed":
            from digat_amd import evaluate
            SC.same((s, i, c), evaluate.shortlist_segments_host(x, np.array(st), m, ids=ids, skip=skip.cpu().numpy()), name)


def test_poisoned_workspace_side_stream_and_back_to_back_calls():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(12)
    m = 257
    x, start, ids, skip = SC.segment_case(rng, m, "seven", True, 50)
    X, ST, I, SK = _t(x), _t(start), _t(ids), _t(skip)
    want = evaluate.shortlist_segments_host(x, start, m, ids=ids, skip=skip)
    first = evaluate.shortlist_segments(X, ST, m, ids=I, skip=SK)
    second = evaluate.shortlist_segments(X, ST, m, ids=I, skip=SK)            # back to back, one workspace
    SC.same(first, want, "first")
    SC.same(second, want, "second")
    need = int(_lib.lib().digat_shortlist_segments_workspace_bytes(len(x), len(start) - 1, m))
    _lib.workspace(need, _dev(), "shortlist").fill_(0xFF)
    SC.same(evaluate.shortlist_segments(X, ST, m, ids=I, skip=SK), want, "poisoned workspace")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = evaluate.shortlist_segments(X, ST, m, ids=I, skip=SK)
        b = evaluate.shortlist_segments(X, ST, m, ids=I, skip=SK)
    side.synchronize()
    SC.same(a, want, "side stream")
    SC.same(b, want, "side stream, second call")
    # the dot entry: the same three, on a pool with more than one chunk and more than one slab
    G, N, P, d, m = 5, 2 * SC.CHUNK, SC.CHUNK + 9, 37, 300
    u, v = rng.standard_normal((G, d)).astype(np.float32), rng.standard_normal((N, d)).astype(np.float32)
    pool = rng.integers(0, N, size=P).astype(np.int64)
    sk = np.stack([pool[rng.integers(0, P, size=50)] for _ in range(G)])
    U, V, PL, SKD = _t(u), _t(v), _t(pool), _t(sk)
    want = evaluate.dot_shortlist_host(evaluate.dot_scores(U, V, pool=PL).cpu().numpy(), m, pool=pool, skip=sk)
    SC.same(evaluate.dot_shortlist(U, V, m, pool=PL, skip=SKD, slab_users=2), want, "dot, first")
    SC.same(evaluate.dot_shortlist(U, V, m, pool=PL, skip=SKD, slab_users=2), want, "dot, second")
    _lib.workspace(int(_lib.lib().digat_dot_shortlist_workspace_bytes(G, P, m, 2)), _dev(), "dot_shortlist").fill_(0xFF)
    SC.same(evaluate.dot_shortlist(U, V, m, pool=PL, skip=SKD, slab_users=2), want, "dot, poisoned workspace")
    with torch.cuda.stream(side):
        c = evaluate.dot_shortlist(U, V, m, pool=PL, skip=SKD, slab_users=2)
    side.synchronize()
    SC.same(c, want, "dot, side stream")
    # the Python entries' refusals
    with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
        evaluate.shortlist_segments(X, ST, 1025)
    with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
        evaluate.dot_shortlist(U, V, 1025)
    with pytest.raises(ValueError, match="slab_users"):
        evaluate.dot_shortlist(U, V, 300, slab_users=0)
    with pytest.raises(ValueError, match="k must be"):
        evaluate.topk_segments(X, ST, 129)
    empty = evaluate.dot_shortlist(U, V, m, pool=_t(np.zeros(0, dtype=np.int64)))
    assert empty[2].tolist() == [0] * G and (empty[1] == -1).all() and tuple(empty[0].shape) == (G, m)


def _dot_case(rng, G, P, d, pool, skip):
    N = P + 37 if pool else P
    users, news = rng.standard_normal((G, d)).astype(np.float32), rng.standard_normal((N, d)).astype(np.float32)
    if d == 1:                                        # a handful of values: every list is full of ties
        users, news = rng.integers(1, 3, size=(G, d)).astype(np.float32), rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    pl = rng.integers(0, N, size=P).astype(np.int64) if pool else None                   # unsorted, with repeats
    sk = None
    if skip:
        src = pl if pool else np.arange(P, dtype=np.int64)
        sk = np.stack([src[rng.integers(0, P, size=50)] for _ in range(G)])
    return users, news, pl, sk


@pytest.mark.parametrize("m", [129, 1024])
def test_dot_shortlist_equals_the_host_contract_on_dot_scores(m):
    from digat_amd import evaluate
    rng = np.random.default_rng(m)
    Gs, ds = (1, 3, 65, 130), (1, 37, 400)
    Ps = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 16385)
    seen = set()
    for n, P in enumerate(Ps):
        G, d = Gs[(n + (m == 1024)) % 4], ds[n % 3]
        seen.add((G, d))
        for pool in (False, True):
            for skip in (False, True):
                users, news, pl, sk = _dot_case(rng, G, P, d, pool, skip)
                U, V, PL, SK = _t(users), _t(news), _t(pl), _t(sk)
                S = evaluate.dot_scores(U, V, pool=PL).cpu().numpy()
                want = evaluate.dot_shortlist_host(S, m, pool=pl, skip=sk)
                got = evaluate.dot_shortlist(U, V, m, pool=PL, skip=SK)
                SC.same(got, want, (G, P, d, m, pool, skip))
                if not skip:
                    assert (want[2] == min(m, P)).all()
                if pool and skip:
                    assert len(np.unique(pl)) < P or P < 3
                    for slab in (1, 64, 100):
                        SC.same(evaluate.dot_shortlist(U, V, m, pool=PL, skip=SK, slab_users=slab), want, (G, P, d, m, "slab", slab))
                    for k in (10, 128):
                        s, i, c = _host(evaluate.dot_topk(U, V, k, pool=PL, skip=SK))
                        SC.same((want[0][:, :k], want[1][:, :k], np.minimum(want[2], k).astype(np.int32)), (s, i, c), (G, P, d, m, "dot_topk", k))
    assert {g for g, _ in seen} == set(Gs) and {d for _, d in seen} == set(ds)


@pytest.mark.parametrize("m", [129, 1024])
def test_dot_rank_below_m_is_the_slot_of_the_shortlist(m):
    """Every pool position a target: ``rank < m`` holds exactly when slot ``rank`` of the user's list holds that element."""
    from digat_amd import evaluate
    rng = np.random.default_rng(21)
    G, P, d = 3, 2049, 37
    users, news, pl, sk = _dot_case(rng, G, P, d, True, True)
    news[:, :] = np.round(news * 2) / 2                              # half-integers: ties, decided by the pool position
    users[:, :] = np.round(users)
    U, V, PL, SK = _t(users), _t(news), _t(pl), _t(sk)
    s, i, c = _host(evaluate.dot_shortlist(U, V, m, pool=PL, skip=SK, slab_users=2))
    target_pos = np.tile(np.arange(P, dtype=np.int64), G)
    rank, score = (t.cpu().numpy() for t in evaluate.dot_rank(U, V, target_pos, np.arange(G + 1, dtype=np.int64) * P, pool=PL, skip=SK))
    rank, score = rank.reshape(G, P), score.reshape(G, P)
    for g in range(G):
        inside = (rank[g] >= 0) & (rank[g] < m)
        assert int(inside.sum()) == int(c[g]) == min(m, int((rank[g] >= 0).sum()))
        pos = np.flatnonzero(inside)
        assert np.array_equal(i[g, rank[g, pos]], pl[pos]) and np.array_equal(SC.bits(s[g, rank[g, pos]]), SC.bits(score[g, pos]))
        assert len(np.unique(SC.bits(s[g, :c[g]]))) < c[g], "ties inside the list"


# ---------------------------------------------------------------------------------------------------------------------
# nrms.shortlist on the device, and into the re-rank
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_shortlist_on_the_device(pre):
    from digat_amd import evaluate, nrms
    m, dev, inp = D.model(pre, _dev()), SC.dev_set(_dev()), SC.inputs()
    users = np.arange(SC.USERS)
    hist, mask = inp["history_ids"], inp["history_mask"].astype(bool)
    with torch.no_grad():
        _, aug = nrms.news_caches(m, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask)
    user = nrms.user_vectors(m, dev, users, batch_size=4)
    skip = np.where(mask, hist, 0)
    # a shared pool: the host contract on dot_scores of the device's own vectors
    pool = np.arange(1, SC.NEWS, dtype=np.int64)
    S = evaluate.dot_scores(user, aug, pool=_t(pool)).cpu().numpy()
    for width in (300, 1024):
        ids, scores, count = nrms.shortlist(m, dev, users, m=width, batch_size=4)
        assert ids.is_cuda and ids.dtype == torch.int64 and scores.dtype == torch.float32 and count.dtype == torch.int32
        SC.same((scores, ids, count), evaluate.dot_shortlist_host(S, width, pool=pool, skip=skip), (pre, width))
    free = nrms.shortlist(m, dev, users, m=300, exclude_history=False)
    SC.same((free[1], free[0], free[2]), evaluate.dot_shortlist_host(S, 300, pool=pool), (pre, "candidates at their word"))
    for a, b in zip(nrms.shortlist(m, dev, users, m=128), nrms.recommend(m, dev, users, k=128)):
        assert torch.equal(a, b), "up to 128 the lists are recommend's"
    # per-user lists: the host contract on row_logits of the device's own vectors
    rng = np.random.default_rng(2)
    lens = [12, 0, 150, 400, 1500, 1]
    lists = [rng.integers(0, SC.NEWS, size=n).astype(np.int64) for n in lens]
    flat, start = np.concatenate(lists), np.r_[0, np.cumsum(lens)].astype(np.int64)
    row_user = np.repeat(users, lens)
    rows = nrms.row_logits(aug[_t(flat)], user[_t(row_user)]).cpu().numpy()
    ids, scores, count = nrms.shortlist(m, dev, users, candidates=(flat, start), m=140)
    SC.same((scores, ids, count), evaluate.shortlist_segments_host(rows, start, 140, ids=flat, skip=skip), (pre, "lists"))
    assert count.tolist()[1] == 0 and int(count[4]) == 140


@functools.lru_cache(maxsize=None)
def _corpus():
    from digat_amd import synthetic
    kw, depth = synthetic.DEVSET_FIXTURES["devset_tiny"]
    spec = synthetic.SynthSpec(**kw)
    return spec, synthetic.make_corpus(spec), depth


def test_retrieve_300_then_rerank_10():
    """NRMS retrieves 300 of devset_tiny's 512 news per user, DIGAT re-ranks them to 10, and both stages are scored on the same
    targets by list_ranks + rank_metrics."""
    from digat_amd import evaluate, nrms, synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    spec, corpus, depth = _corpus()
    assert spec.news_num == SC.NEWS
    first, dev = D.model("nrms", _dev()), SC.dev_set(_dev())
    users = np.arange(SC.USERS)
    ids, scores, count = nrms.shortlist(first, dev, users, m=300)
    assert tuple(ids.shape) == (SC.USERS, 300) and (count == 300).all()
    flat, start = nrms.candidates_csr(ids, count)
    assert start.tolist() == (np.arange(SC.USERS + 1) * 300).tolist() and flat.tolist() == ids.reshape(-1).tolist()
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    second = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, depth, seed=spec.seed + 1, bias_std=0.05)
    second.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    second = second.to(_dev()).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, _dev())
    top, top_scores, top_count = util.recommend(second, dc, users, (flat, start), k=10, exclude_history=False, batch_size=256)
    assert tuple(top.shape) == (SC.USERS, 10) and (top_count == 10).all()
    listed = ids.cpu().numpy()
    for g in range(SC.USERS):
        assert set(top[g].tolist()) <= set(listed[g].tolist()) and len(set(top[g].tolist())) == 10
    # targets: per user slot 0 and slot 299 of the shortlist, and a news that is not in it
    outside = [int(np.setdiff1d(np.arange(1, SC.NEWS), listed[g])[0]) for g in range(SC.USERS)]
    targets = np.stack([listed[:, 0], listed[:, 299], np.array(outside)], axis=1).reshape(-1)
    target_start = np.arange(SC.USERS + 1, dtype=np.int64) * 3
    r1 = evaluate.list_ranks(ids, count, targets, target_start).cpu().numpy()
    assert r1.reshape(SC.USERS, 3).tolist() == [[0, 299, -1]] * SC.USERS
    one = evaluate.rank_metrics(r1, target_start, ks=(10, 300))
    assert one["recall@10"] == pytest.approx(1 / 3) and one["recall@300"] == pytest.approx(2 / 3) and one["not_ranked"] == SC.USERS
    r2 = evaluate.list_ranks(top, top_count, targets, target_start).cpu().numpy()
    two = evaluate.rank_metrics(r2, target_start, ks=(10, 300))
    assert (r2.reshape(SC.USERS, 3)[:, 2] == -1).all() and two["recall@10"] == two["recall@300"] <= 2 / 3
