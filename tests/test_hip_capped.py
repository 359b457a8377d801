"""GPU suite: the exposure-capped top-k kernels (``digat_capped_prepare`` / ``digat_capped_rounds`` / ``digat_capped_emit``) and
``recommend(exposure_cap=)`` on them.  The assignment is unique and is reached by comparisons alone, so the device is held EXACTLY
to the host contract (``evaluate.capped_select_host``): ids, score bits, count, slots, the fill and ``rounds`` — on the cases
tests/test_capped_cpu.py holds to be stable and order-independent (same generator, same seeds: tests/capped_common.py)."""
import functools
import types

import numpy as np
import pytest
import torch

import capped_common as K
import dot_topk_common as D

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.array(x)).to(_dev())             # a copy: the shared cases are read-only


def _cap(capv):
    return _t(capv) if isinstance(capv, np.ndarray) else capv


def _identical(a, b, what=""):
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and np.array_equal(K.bits(x.cpu().numpy()), K.bits(y.cpu().numpy())), what
    assert a[4] == b[4], what


@pytest.mark.parametrize("cap", K.CAPS)
@pytest.mark.parametrize("G,M,k,P", K.CASES)
def test_assignment_is_exact_against_the_twin(G, M, k, P, cap):
    from digat_amd import evaluate
    (ids, scores, count, _), capv, want = K.case(G, M, k, P, cap)
    got = evaluate.capped_select(_t(ids), _t(scores), _t(count), k, _cap(capv), P)
    assert all(t.is_cuda for t in got[:4]) and isinstance(got[4], int)
    K.same(got, want, (G, M, k, P, cap))


@pytest.mark.parametrize("G,M,k,P,cap", [(65, 65, 1, 30, 2), (33, 257, 10, 300, 1), (300, 1024, 10, 1100, 2), (65, 1024, 128, 1500, "array")])
def test_a_given_priority_and_no_count(G, M, k, P, cap):
    from digat_amd import evaluate
    (ids, scores, count, pr), capv, want = K.case(G, M, k, P, cap, True)
    got = evaluate.capped_select(_t(ids), _t(scores), _t(count), k, _cap(capv), P, priority=_t(pr))
    K.same(got, want, "priority")
    got = evaluate.capped_select(_t(ids), _t(scores), None, k, _cap(capv), P, priority=_t(pr))
    K.same(got, evaluate.capped_select_host(ids, scores, None, k, capv, P, priority=pr, max_rounds=K.ROUND_LIMIT), "count None")


@pytest.mark.parametrize("G,M,k,P,cap", [(33, 257, 10, 300, 1), (300, 64, 10, 200, 7), (65, 1024, 128, 1500, 7)])
def test_rounds_per_sync_changes_nothing_and_two_calls_agree(G, M, k, P, cap):
    from digat_amd import evaluate
    (ids, scores, count, _), capv, want = K.case(G, M, k, P, cap)
    assert want[4] >= 3, "the case takes several rounds"
    args = (_t(ids), _t(scores), _t(count), k, _cap(capv), P)
    first = evaluate.capped_select(*args)
    K.same(first, want, "default")
    _identical(evaluate.capped_select(*args), first, "two calls")
    for rps in (1, 4, 7):
        got = evaluate.capped_select(*args, rounds_per_sync=rps)
        K.same(got, want, ("rounds_per_sync", rps))
    assert evaluate.capped_select(*args, max_rounds=want[4])[4] == want[4], "max_rounds = the rounds needed is enough"


def test_max_rounds_raises_where_the_twin_needs_more():
    from digat_amd import evaluate
    (ids, scores, count, _), capv, want = K.case(33, 257, 10, 300, 1)
    assert want[4] > 1
    for rps in (1, 4):
        with pytest.raises(RuntimeError, match="max_rounds"):
            evaluate.capped_select(_t(ids), _t(scores), _t(count), 10, capv, 300, rounds_per_sync=rps, max_rounds=1)
    with pytest.raises(RuntimeError, match="max_rounds"):
        evaluate.capped_select(_t(ids), _t(scores), _t(count), 10, capv, 300, rounds_per_sync=4, max_rounds=want[4] - 1)


def test_reductions_nobody_and_a_side_stream():
    from digat_amd import evaluate
    G, M, k, P = 65, 64, 10, 50
    ids, scores, count, _ = K.make_lists(K.seed_of(G, M, k, P), G, M, P)
    IDS, SC, CNT = _t(ids), _t(scores), _t(count)
    for cap in (G, 0):
        K.same(evaluate.capped_select(IDS, SC, CNT, k, cap, P), evaluate.capped_select_host(ids, scores, count, k, cap, P), ("cap", cap))
    nobody = evaluate.capped_select(IDS[:0], SC[:0], CNT[:0], k, 1, P)
    assert [tuple(t.shape) for t in nobody[:4]] == [(0, k), (0, k), (0,), (0, k)] and all(t.is_cuda for t in nobody[:4])
    assert nobody[4] == evaluate.capped_select_host(ids[:0], scores[:0], count[:0], k, 1, P)[4]
    no_news = evaluate.capped_select(IDS, SC, CNT, k, 1, 0)
    K.same(no_news, evaluate.capped_select_host(ids, scores, count, k, 1, 0), "P = 0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = evaluate.capped_select(IDS, SC, CNT, k, 2, P)
    side.synchronize()
    K.same(on_side, evaluate.capped_select_host(ids, scores, count, k, 2, P), "side stream")
    with pytest.raises(ValueError, match="k must be"):
        evaluate.capped_select(IDS, SC, CNT, 129, 1, P)
    with pytest.raises(ValueError, match="cap must"):
        evaluate.capped_select(IDS, SC, CNT, k, -1, P)
    with pytest.raises(ValueError, match="cap must"):
        evaluate.capped_select(IDS, SC, CNT, k, torch.zeros(P, device=_dev()), P)
    with pytest.raises(ValueError, match="rounds_per_sync"):
        evaluate.capped_select(IDS, SC, CNT, k, 1, P, rounds_per_sync=0)


def test_c_entries_write_the_outputs_and_the_stated_workspace_only():
    """The three entries by hand, in buffers with guard regions: the workspace of ``digat_capped_select_workspace_bytes`` and every
    output are embedded in tensors full of a pattern; behind the call the pattern stands on both sides of each, the inputs are
    unchanged and the outputs are the twin's."""
    from digat_amd import _lib
    G, M, k, P, cap = 65, 65, 1, 30, 2
    (ids, scores, count, _), capv, want = K.case(G, M, k, P, cap)
    IDS, SC, CNT = _t(ids), _t(scores), _t(count)
    inputs = [t.clone() for t in (IDS, SC, CNT)]
    L, dev, pad = _lib.lib(), _dev(), 256
    need = int(L.digat_capped_select_workspace_bytes(G, M))
    assert need % 8 == 0
    ws = torch.full((pad + need + pad,), 0xA5, dtype=torch.uint8, device=dev)
    tail = (ws[pad:].data_ptr(), need, _lib.stream_ptr())
    _lib.check(L.digat_capped_prepare(IDS.data_ptr(), SC.data_ptr(), None, CNT.data_ptr(), G, M, P, *tail), "digat_capped_prepare")
    words, perm = torch.sort(ws[pad:pad + G * M * 8].view(torch.int64).clone(), stable=True)
    perm = perm.to(torch.int32)
    caps = torch.full((P,), cap, dtype=torch.int32, device=dev)
    bounds = torch.searchsorted(words >> 32, torch.arange(P + 1, dtype=torch.int64, device=dev))
    length = bounds[1:] - bounds[:-1]
    binding = torch.nonzero(length > caps).view(-1)
    n_seg, rounds = int(binding.shape[0]), want[4] + 2                                     # two rounds past the fixed point
    assert n_seg > 0
    guarded = lambda t, fill: torch.cat([torch.full((pad,), fill, dtype=t.dtype, device=dev), t, torch.full((pad,), fill, dtype=t.dtype, device=dev)])
    seg_begin = guarded(bounds[:-1][binding].to(torch.int32), -5)
    seg_cap = guarded(caps[binding], -5)
    seg_live = guarded(length[binding].to(torch.int32), -5)
    counter = guarded(torch.zeros(rounds, dtype=torch.int32, device=dev), -9)
    frozen = [t.clone() for t in (perm, seg_begin, seg_cap)]
    _lib.check(L.digat_capped_rounds(G, M, k, perm.data_ptr(), seg_begin[pad:].data_ptr(), seg_cap[pad:].data_ptr(), seg_live[pad:].data_ptr(),
                                     n_seg, counter[pad:].data_ptr(), rounds, *tail), "digat_capped_rounds")
    out_i = torch.full((pad + G * k + pad,), 77, dtype=torch.int64, device=dev)
    out_s = torch.full((pad + G * k + pad,), 123.0, dtype=torch.float32, device=dev)
    out_c = torch.full((pad + G + pad,), 55, dtype=torch.int32, device=dev)
    out_p = torch.full((pad + G * k + pad,), 66, dtype=torch.int32, device=dev)
    _lib.check(L.digat_capped_emit(IDS.data_ptr(), SC.data_ptr(), G, M, k, out_i[pad:].data_ptr(), out_s[pad:].data_ptr(), out_c[pad:].data_ptr(),
                                   out_p[pad:].data_ptr(), *tail), "digat_capped_emit")
    torch.cuda.synchronize()
    assert (ws[:pad] == 0xA5).all() and (ws[pad + need:] == 0xA5).all(), "the workspace's guards"
    for t, n, fill in ((out_i, G * k, 77), (out_s, G * k, 123.0), (out_c, G, 55), (out_p, G * k, 66), (seg_live, n_seg, -5),
                       (counter, rounds, -9)):
        assert (t[:pad] == fill).all() and (t[pad + n:] == fill).all()
    assert all(torch.equal(a, b) for a, b in zip(frozen, (perm, seg_begin, seg_cap))), "perm and the segment table are read only"
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(inputs, (IDS, SC, CNT))), "inputs are read only"
    c = counter[pad:pad + rounds].cpu().numpy()
    assert (c[:want[4] - 1] > 0).all() and (c[want[4] - 1:] == 0).all(), "counter[r]: what round r rejected; nothing from the fixed point on"
    raw = (out_i[pad:pad + G * k].view(G, k), out_s[pad:pad + G * k].view(G, k), out_c[pad:pad + G], out_p[pad:pad + G * k].view(G, k), want[4])
    K.same(raw, want, "raw calls")
    live = seg_live[pad:pad + n_seg].cpu().numpy()
    assert (live >= 0).all() and (live <= length[binding].cpu().numpy()).all() and (live < length[binding].cpu().numpy()).any()


# ---------------------------------------------------------------------------------------------------------------------
# recommend(exposure_cap=) end to end
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus():
    from digat_amd import synthetic
    kw, depth = synthetic.DEVSET_FIXTURES["devset_tiny"]
    spec = synthetic.SynthSpec(**kw)
    return spec, synthetic.make_corpus(spec), depth


def _model():
    from digat_amd import synthetic
    from digat_amd.model import Model, PrecomputedNewsEncoder
    spec, corpus, depth = _corpus()
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, depth, seed=spec.seed + 1, bias_std=0.05)
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return model.to(_dev()).eval()


def _twin_on(short, k, cap, P):
    from digat_amd import evaluate
    return evaluate.capped_select_host(short[0].cpu().numpy(), short[1].cpu().numpy(), short[2].cpu().numpy(), k, cap, P)


def test_digat_recommend_with_exposure_cap_end_to_end():
    from digat_amd import util
    spec, corpus, _ = _corpus()
    model, dc = _model(), util.DeviceCorpus.from_numpy(corpus, _dev())
    users, pool, k, N = np.arange(64), np.arange(1, spec.news_num, dtype=np.int64), 10, spec.news_num
    plain = util.recommend(model, dc, users, pool, k, batch_size=256)
    again = util.recommend(model, dc, users, pool, k, batch_size=256, exposure_cap=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    assert len(users) * k > N and np.bincount(plain[0].cpu().numpy().reshape(-1).clip(0)).max() >= 2, "640 picks of 511 news: a cap of 1 binds"
    for cap, shortlist, wide in ((2, None, 80), (1, 200, 200), (len(users), None, 80)):
        short = (util.recommend(model, dc, users, pool, wide, batch_size=256) if wide <= 128 else
                 util.recommend_lists(model, dc, users, pool, wide, batch_size=256))
        got = util.recommend(model, dc, users, pool, k, batch_size=256, exposure_cap=cap, shortlist=shortlist)
        assert got[0].is_cuda and got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        want = _twin_on(short, k, cap, N)
        K.same(tuple(got) + (want[3], want[4]), want, ("DIGAT", cap, wide))
        shown = got[0].cpu().numpy()
        assert np.bincount(shown[shown >= 0], minlength=N).max() <= cap
        if cap == len(users):
            assert all(torch.equal(a, b) for a, b in zip(got, plain)), "a cap of G: the plain list"
    with pytest.raises(ValueError, match="does not combine"):
        util.recommend(model, dc, users, pool, k, batch_size=256, exposure_cap=2, diversity=0.3)


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_exposure_cap_end_to_end(pre):
    from digat_amd import nrms
    m, dev = D.model(pre, _dev()), D.dev_set(_dev())
    users, k = np.arange(D.USERS), 5
    wide = nrms.recommend(m, dev, users, k=40, batch_size=4)
    got = nrms.recommend(m, dev, users, k=k, batch_size=4, exposure_cap=2)
    want = _twin_on(wide, k, 2, D.NEWS)
    K.same(tuple(got) + (want[3], want[4]), want, (pre, "cap 2"))
    pool = np.tile(np.arange(1, D.NEWS, dtype=np.int64), 3)            # every news three times: a list names an id more than once
    long = nrms.shortlist(m, dev, users, candidates=pool, m=200, batch_size=4)
    got = nrms.recommend(m, dev, users, candidates=pool, k=k, batch_size=4, exposure_cap=3, shortlist=200)
    want = _twin_on(long, k, 3, D.NEWS)
    K.same(tuple(got) + (want[3], want[4]), want, (pre, "shortlist 200"))
