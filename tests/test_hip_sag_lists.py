"""GPU suite for the SAG built from sentence embeddings: ``digat_sag_similar_lists`` (``sag_lists_kernel``) bit for bit against
the numpy walk over ``digat_sag_cos_topk``'s average top-k, ``build_similarity`` on tests/golden/sag_tiny against what the
reference made of it (tests/golden/sag_tiny_golden.npz), and the loader and ``main`` with ``semantic_embedding_root``."""
import numpy as np
import pytest
import torch

from sag_common import DATASETS, FIXTURE, HOPS, LOAD, TOP_M, corpus_inputs, embedding_root, minted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_shared = {}


def group_structure(n, m, seed):
    """Seeded title groups: query groups of 1-4 news, one of 300 (more than one pass of the 256 threads), news rows shuffled over
    [1, news_num) with some rows in no group; corpus group j is a non-empty part of query group ``match[j]``, so some query news are
    in no corpus group.  Returns (group_start, group_member, corpus_start, corpus_member, match, news_num)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 5, size=n)
    sizes[rng.integers(0, n)] = 300
    total = int(sizes.sum())
    news_num = total + 1 + 37                                          # the padding row and 37 news of other categories
    rows = rng.permutation(np.arange(1, news_num))[:total].astype(np.int32)
    group_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert m <= n
    match = rng.permutation(n)
    if m > 1:                                                          # the 300-news group is in the corpus: a long skip scan
        big = int(np.argmax(sizes))
        match = np.concatenate([[big], match[match != big]])
    match = match[:m]
    corpus_start, corpus_member = [0], []
    for g in match:
        members = rows[group_start[g]:group_start[g + 1]]
        keep = members[rng.random(len(members)) < 0.6]
        keep = keep if len(keep) else members[:1]
        corpus_member.extend(rng.permutation(keep).tolist())
        corpus_start.append(len(corpus_member))
    return group_start, rows, np.asarray(corpus_start, dtype=np.int32), np.asarray(corpus_member, dtype=np.int32), match, news_num


@pytest.mark.parametrize("n,m,dim,top_M", [(300, 200, 32, 5), (700, 333, 48, 7),     # K = 8
                                           (200, 150, 16, 31),                       # K = 32
                                           (40, 3, 32, 5),                           # M' = 2, K = 4
                                           (50, 1, 16, 5),                           # M' = 0: the stop test that never fires
                                           (4500, 500, 64, 3),                       # two query chunks, row0 != 0
                                           (120, 100, 32, 12)])                      # K = 16
def test_lists_kernel_equals_the_host_walk_over_cos_topk_bit_for_bit(n, m, dim, top_M):
    from digat_amd import construct_SAG, synthetic
    gs, gm, cs, cm, match, news_num = group_structure(n, m, seed=n + m)
    title, content = synthetic.make_semantic_embeddings(n, dim, seed=n + m + 1)
    # a corpus group carries the embeddings of the query group it is part of: cosine 1, the first of its k best, and skipped by its members
    embeddings = [torch.from_numpy(x).to(DEV) for x in (title, content, title[match], content[match])]
    k = min(top_M, m - 1) + 1
    values, indices = construct_SAG.cos_topk_device(*embeddings, top_M=top_M)
    assert tuple(values.shape) == (5, n, k)
    sentinel = (-7, -3.0, -1)
    want = tuple(np.full(shape, fill, dtype=dtype) for shape, fill, dtype in
                 zip(((news_num, top_M), (news_num, top_M), (news_num,)), sentinel, (np.int32, np.float32, np.int32)))
    construct_SAG.similar_news_lists_host(values[4].cpu().numpy(), indices[4].cpu().numpy(), k, gs, gm, cs, cm, top_M, news_num, out=want)
    got = tuple(torch.from_numpy(w).to(DEV).fill_(fill) for w, fill in zip(want, sentinel))
    back = construct_SAG.similar_news_lists_device(*embeddings, top_M, gs, gm, cs, cm, news_num, out=got)
    torch.cuda.synchronize()
    assert all(b.data_ptr() == g.data_ptr() for b, g in zip(back, got))
    index, cos, length = (t.cpu().numpy() for t in got)
    assert np.array_equal(length, want[2])
    assert np.array_equal(index, want[0])
    assert np.array_equal(cos.view(np.int32), want[1].view(np.int32))                # the same bits
    # what the shapes are there for
    outside = np.setdiff1d(np.arange(news_num), gm)
    assert len(outside) == 38 and (length[outside] == -1).all() and (index[outside] == -7).all() and (cos[outside] == -3.0).all()
    written = length[gm]
    stop = k - 1
    assert written.min() >= 0 and written.max() == max(stop, 1 if m == 1 else 0)
    in_corpus = np.isin(gm, cm)
    if m == 1:
        assert (written[in_corpus] == 0).all() and (written[~in_corpus] == 1).all()   # M' = 0: one entry unless it is the news's own group
    else:
        assert (written == stop).all() and in_corpus.any() and (~in_corpus).any()
        idx4 = indices[4].cpu().numpy()
        hit = [(idx4[g] == j).any() for j, g in enumerate(match)]                    # a group's twin in the corpus is among its k best,
        assert np.mean(hit) > 0.5                                                    # so the skip test fired for that group's corpus members
    live = np.arange(top_M)[None] < written[:, None]
    assert np.isin(index[gm][live], cm[cs[:-1]]).all()                               # representatives only


def test_lists_mirror_refuses_cpu_tensors_oversized_k_and_bad_outputs():
    from digat_amd import _lib, construct_SAG
    gs, gm = np.array([0, 1, 2], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    x = torch.zeros(2, 16)
    with pytest.raises(_lib.DigatHipError):
        construct_SAG.similar_news_lists_device(x, x, x, x, 3, gs, gm, gs, gm, 3)
    big = torch.zeros(64, 16, device=DEV)
    many = np.arange(65, dtype=np.int32)
    with pytest.raises(ValueError):
        construct_SAG.similar_news_lists_device(big, big, big, big, 40, many, many[1:], many, many[1:], 65)
    d = x.to(DEV)
    with pytest.raises(ValueError):                                                  # a list array of another news count
        construct_SAG.similar_news_lists_device(d, d, d, d, 3, gs, gm, gs, gm, 3, out=(torch.zeros(2, 3, dtype=torch.int32, device=DEV),
                                                torch.zeros(3, 3, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV)))


def built(dataset):
    """``build_similarity`` on the fixture and the device walk over it, once per dataset type, as numpy arrays."""
    from digat_amd import construct_SAG, synthetic
    if dataset not in _shared:
        news, dictionaries = corpus_inputs()
        lists = construct_SAG.build_similarity(news, dictionaries, embedding_root(dataset), TOP_M, dataset)
        assert all(t.device.type == "cuda" for t in lists)
        graphs = construct_SAG.news_graph_device(*lists, top_M=TOP_M, hop=HOPS, news_node_num=synthetic.news_graph_size(TOP_M, HOPS))
        _shared[dataset] = tuple(t.cpu().numpy() for t in lists + graphs)
    return _shared[dataset]


def keep_rows(dataset):
    """Every news but the two with no text, whose neighbours the reference draws with an unseeded generator."""
    keep = np.ones(len(minted()[dataset + "/sim_len"]), dtype=bool)
    keep[minted()[dataset + "/empty_rows"]] = False
    assert (~keep).sum() == 2
    return keep


@pytest.mark.parametrize("dataset", DATASETS)
def test_build_similarity_on_the_fixture_equals_the_references_lists_and_graphs(dataset):
    g, keep = minted(), keep_rows(dataset)
    sim_index, sim_cos, sim_len, node_ID, graph, mask = built(dataset)
    want_index, want_cos, want_len = (g[dataset + "/" + k] for k in ("sim_index", "sim_cos", "sim_len"))
    err = np.abs(sim_cos[keep] - want_cos[keep]).max()
    print(f"\n[sag_tiny {dataset}] {int(keep.sum())} news, {int(want_len[keep].sum())} list entries, cosine max|diff| {err:.3e}")
    assert np.array_equal(sim_len[keep], want_len[keep])
    assert np.array_equal(sim_index[keep], want_index[keep])          # every entry: the mint tool asserts the cosines' separation
    assert err <= 2e-6                                                 # the project's bound for these cosines (tests/test_sag.py)
    assert node_ID.dtype == np.int32 and np.array_equal(node_ID[keep], g[dataset + "/news_node_ID"][keep])
    assert graph.dtype == bool and np.array_equal(graph[keep], g[dataset + "/news_graph"][keep])
    assert mask.dtype == bool and np.array_equal(mask[keep], g[dataset + "/news_graph_mask"][keep])
    assert mask[keep].sum(axis=1).max() > TOP_M + 1                    # second-hop nodes: the threshold and the top_M - 1 cut were at work
    # the news with no text: a full list of distinct same-category news, not itself, cosine 0
    news, dictionaries = corpus_inputs()
    category_of = {dictionaries["news_ID"][n[0]]: n[1] for n in news}
    for row in np.nonzero(~keep)[0]:
        ids = sim_index[row, :sim_len[row]]
        assert sim_len[row] == TOP_M == len(set(ids.tolist())) and row not in ids and (sim_cos[row] == 0).all()
        assert all(category_of[int(x)] == category_of[int(row)] for x in ids)


@pytest.mark.parametrize("dataset", DATASETS)
def test_loader_builds_the_news_graphs_from_embeddings_and_caches_them(dataset, tmp_path):
    from digat_amd import construct_SAG, mind
    g, keep = minted(), keep_rows(dataset)
    N = g[dataset + "/news_graph"].shape[1]
    kw = dict(LOAD, dataset=dataset, verbose=False)
    corpus = mind.load(FIXTURE, semantic_embedding_root=embedding_root(dataset), data_cache=str(tmp_path / "cache"), **kw)
    assert corpus.news_graph_source == "embeddings" and corpus.embedding_news is None
    want_mask = g[dataset + "/news_graph_mask"].copy()
    want_mask[:, 0] = False
    assert np.array_equal(corpus.news_node_ID[keep], g[dataset + "/news_node_ID"][keep])
    assert np.array_equal(corpus.news_graph[keep], (g[dataset + "/news_graph"] | np.identity(N, dtype=bool)[None])[keep])
    assert np.array_equal(corpus.news_graph_mask[keep], want_mask[keep]) and not corpus.news_graph_mask[:, 0].any()
    assert np.array_equal(corpus.news_node_ID, built(dataset)[3])      # ... and every row is the direct build's (the same seed)
    again = mind.load(FIXTURE, semantic_embedding_root=embedding_root(dataset), data_cache=str(tmp_path / "cache"), **kw)
    assert again.news_graph_source == "embeddings" and again.header() == corpus.header() and again.header()["version"] == mind.CACHE_VERSION
    for name in ("news_node_ID", "news_graph", "news_graph_mask"):
        assert np.array_equal(getattr(again, name), getattr(corpus, name)), name
    deferred = mind.load(FIXTURE, semantic_embedding_root=embedding_root(dataset), defer_news_graphs=True, **kw)
    assert deferred.news_graph is None and deferred.embedding_news is not None
    assert np.array_equal(deferred.train.news_graph, corpus.news_graph) and deferred.news_graph_source == "embeddings"
    # a similarity file written by ``build`` and read back through the existing path gives the same graphs
    path = str(tmp_path / "similarity.json")
    construct_SAG.main(["build", "--data_root", FIXTURE, "--embedding_root", embedding_root(dataset), "--top_M", str(TOP_M),
                        "--dataset", dataset, "--output", path])
    from_file = mind.load(FIXTURE, similarity_file=path, **kw)
    assert from_file.news_graph_source == "similarity"
    for name in ("news_node_ID", "news_graph", "news_graph_mask"):
        assert np.array_equal(getattr(from_file, name), getattr(corpus, name)), name
    # a similarity file wins over the embeddings, as the artefact wins over both
    both = mind.load(FIXTURE, similarity_file=path, semantic_embedding_root=embedding_root(dataset), **kw)
    assert both.news_graph_source == "similarity"


def test_main_trains_on_the_fixture_with_graphs_from_embeddings(tmp_path, capsys):
    from digat_amd.main import main
    main(["--mode", "train", "--max_steps", "2", "--data_root", FIXTURE, "--semantic_embedding_root", embedding_root("small"),
          "--dataset", "MIND-small", "--news_encoder", "MSA", "--MSA_head_num", "4",
          "--MSA_head_dim", "16", "--word_embedding_dim", "20", "--attention_dim", "32", "--graph_depth", "2", "--max_history_num", "10",
          "--max_title_length", "8", "--word_threshold", "1", "--SAG_hops", str(HOPS), "--SAG_neighbors", str(TOP_M), "--batch_size", "8"])
    out = capsys.readouterr().out
    assert "mind: news graphs from embeddings" in out and "AUC : " in out
    metrics = [float(line.split(" : ")[1]) for line in out.splitlines() if line.split(" : ")[0] in ("AUC", "MRR", "nDCG@5", "nDCG@10")]
    assert len(metrics) == 4 and all(np.isfinite(metrics)), out
