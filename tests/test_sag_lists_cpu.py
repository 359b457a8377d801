"""CPU suite for the SAG's middle steps (construct_SAG.py:13-92 and :217-446): ``news_meta``, the similar-news walk's numpy
yardstick, the Appendix B table and the similarity file, against what the reference made of tests/golden/sag_tiny
(tests/golden/sag_tiny_golden.npz, tools/mint_sag_golden.py); the new C entry's declaration and the CSR validation."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from sag_common import DATASETS, TOP_M, categories_with_corpus, corpus_inputs, minted, minted_json

MODES = ("full", "corpus")


def host_lists(dataset, seed=0):
    """The fixture's lists from the golden's OWN average top-k through the numpy walk, the news with no text drawn on the host."""
    from digat_amd import construct_SAG
    news, dictionaries = corpus_inputs()
    g, news_ID = minted(), dictionaries["news_ID"]
    rows, has_corpus = construct_SAG.category_rows(news)
    out = (np.zeros((len(news_ID), TOP_M), dtype=np.int32), np.zeros((len(news_ID), TOP_M), dtype=np.float32), np.zeros(len(news_ID), dtype=np.int32))
    rng = np.random.default_rng(seed)
    assert [c for c in dictionaries["category"] if c in has_corpus] == categories_with_corpus(dataset)
    for category in categories_with_corpus(dataset):
        full, corpus, gs, gm, cs, cm = construct_SAG.category_tables(rows[category], news_ID, dataset)
        values, indices = g["%s/%s/avg_values" % (dataset, category)], g["%s/%s/avg_indices" % (dataset, category)]
        assert values.shape == (len(full[2]), min(TOP_M, len(corpus[2]) - 1) + 1)
        construct_SAG.validate_csr(gs, gm, len(full[2]), len(news_ID), "query groups")
        construct_SAG.validate_csr(cs, cm, len(corpus[2]), len(news_ID), "corpus groups", nonempty=True)
        construct_SAG.similar_news_lists_host(values, indices, values.shape[1], gs, gm, cs, cm, TOP_M, len(news_ID), out=out)
        for row, picked in construct_SAG.empty_news_lists(rng, full[4], [r[1] for r in rows[category]], news_ID, TOP_M):
            out[0][row, :len(picked)], out[1][row], out[2][row] = picked, 0.0, len(picked)
    return out


@pytest.mark.parametrize("dataset", DATASETS)
def test_news_meta_equals_the_references_five_items(dataset):
    from digat_amd import construct_SAG
    rows, has_corpus = construct_SAG.category_rows(corpus_inputs()[0])
    checked = 0
    for category in minted_json("category"):
        for mode in MODES:
            key = "%s/%s/meta_%s" % (dataset, category, mode)
            assert (key in minted()) == (category in has_corpus)
            if category not in has_corpus:
                continue
            want = minted_json(key)
            got = construct_SAG.news_meta(rows[category], mode, construct_SAG.excludes_test(dataset))
            for name, item in zip(("news_dict", "news_dict_inv", "titles", "contents", "empty_news_IDs"), got):
                assert item == want[name], (category, mode, name)
                if isinstance(item, dict):
                    assert list(item) == list(want[name]), (category, mode, name)            # the same order, too
            checked += 1
    assert checked == 8
    # the fixture holds what it is meant to: a title group of several news, a news with no text, a content with its title in front
    sports = construct_SAG.news_meta(rows["sports"], "full", False)
    assert max(len(v) for v in sports[1].values()) == 3 and len(sports[4]) == 2
    assert any(c.startswith(t + " ") for t, c in zip(sports[2], sports[3]))
    assert "weather" not in has_corpus and len(construct_SAG.news_meta(rows["solo"], "corpus", True)[2]) == 1


def test_news_meta_rules_on_a_handful_of_rows():
    from digat_amd.construct_SAG import news_meta
    rows = [("train_dev", "A", "Café One", "first"), ("train_dev", "B", "", "Only Abstract"), ("train_dev", "C", "only title", ""),
            ("train_dev", "D", "", ""), ("test", "E", "CAFÉ one", ""), ("train_dev", "F", "other", "first"), ("train_dev", "A", "again", "x")]
    news_dict, inv, titles, contents, empty = news_meta(rows, "full", True)
    assert titles == ["cafe one", "only abstract", "only title", "other"]
    assert contents == ["cafe one first", "only abstract", "only title", "other first"]          # 'first' is duplicated: title in front
    assert inv == {"0": ["A", "E"], "1": ["B"], "2": ["C"], "3": ["F"]} and news_dict == {"A": 0, "E": 0, "B": 1, "C": 2, "F": 3}
    assert empty == ["D"]
    assert news_meta(rows, "corpus", True)[1]["0"] == ["A"] and news_meta(rows, "corpus", False)[1]["0"] == ["A", "E"]
    with pytest.raises(ValueError):
        news_meta(rows, "test", True)


@pytest.mark.parametrize("dataset", DATASETS)
def test_host_walk_on_the_goldens_own_topk_reproduces_the_aggregated_lists(dataset):
    g = minted()
    sim_index, sim_cos, sim_len = host_lists(dataset)
    empty = g[dataset + "/empty_rows"]
    keep = np.ones(len(sim_len), dtype=bool)
    keep[empty] = False
    assert len(empty) == 2
    assert np.array_equal(sim_len[keep], g[dataset + "/sim_len"][keep])
    assert np.array_equal(sim_index[keep], g[dataset + "/sim_index"][keep])
    assert np.array_equal(sim_cos[keep], g[dataset + "/sim_cos"][keep])                          # the same float32, bit for bit
    # the cases the fixture is there for: the test-only category has empty lists, the one-group corpus (M' = 0) still writes an entry
    news_ID = corpus_inputs()[1]["news_ID"]
    category_of = {n[0]: n[1] for n in corpus_inputs()[0]}
    assert all(sim_len[news_ID[n]] == 0 for n, c in category_of.items() if c == "weather")
    solo = sorted(int(sim_len[news_ID[n]]) for n, c in category_of.items() if c == "solo")
    assert solo == ([0, 0, 1] if dataset == "small" else [1, 1, 1])
    assert sim_len.max() == TOP_M and ((sim_len > 1) & (sim_len < TOP_M)).any()                   # full lists, and the short ones of 'few'


@pytest.mark.parametrize("dataset", DATASETS)
def test_news_with_no_text_get_seeded_same_category_neighbours(dataset):
    news, dictionaries = corpus_inputs()
    news_ID = dictionaries["news_ID"]
    category_of = {news_ID[n[0]]: n[1] for n in news}
    a, b, c = host_lists(dataset, seed=0), host_lists(dataset, seed=0), host_lists(dataset, seed=3)
    for row in minted()[dataset + "/empty_rows"]:
        ids = a[0][row, :a[2][row]]
        assert a[2][row] == TOP_M == len(set(ids.tolist())) and row not in ids                 # 21 sports news: a full list
        assert all(category_of[int(x)] == category_of[int(row)] for x in ids) and (a[1][row] == 0).all()
        assert np.array_equal(ids, b[0][row, :b[2][row]])
    assert any(not np.array_equal(a[0][row], c[0][row]) for row in minted()[dataset + "/empty_rows"])


@pytest.mark.parametrize("A", [3, TOP_M, 8])
def test_semantic_augmented_news_matches_appendix_b(A):
    from digat_amd import construct_SAG
    g, news_ID = minted(), corpus_inputs()[1]["news_ID"]
    sim_index, sim_cos, sim_len = (g["small/" + k] for k in ("sim_index", "sim_cos", "sim_len"))
    augmented = construct_SAG.similarity_dict(sim_index, sim_cos, sim_len, news_ID)
    want = np.zeros((len(news_ID), A), dtype=np.int32)                                         # MIND_corpus.py:113-119
    for n, index in news_ID.items():
        if index > 0:
            for j in range(min(A, len(augmented[n]))):
                want[index][j] = news_ID[augmented[n][j][0]]
    got = construct_SAG.semantic_augmented_news(sim_index, sim_len, A)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    as_tensor = construct_SAG.semantic_augmented_news(torch.from_numpy(sim_index), torch.from_numpy(sim_len), A)
    assert as_tensor.dtype == torch.int32 and np.array_equal(as_tensor.numpy(), want)


def test_similarity_json_round_trips_through_similarity_lists(tmp_path):
    from digat_amd import construct_SAG
    g, news_ID = minted(), corpus_inputs()[1]["news_ID"]
    arrays = tuple(g["large/" + k] for k in ("sim_index", "sim_cos", "sim_len"))
    path = str(tmp_path / "similarity-5.json")
    construct_SAG.write_similarity_json(path, *arrays, news_ID)
    with open(path, encoding="utf-8") as f:
        written = json.load(f)
    assert set(written) == set(news_ID) and written["<PAD>"] == []
    back = construct_SAG.similarity_lists(written, news_ID, TOP_M)
    for got, want in zip(back, arrays):
        assert got.dtype == want.dtype and np.array_equal(got, want)


def test_embedding_files_are_held_to_news_metas_row_count(tmp_path):
    from digat_amd import construct_SAG
    d = tmp_path / "semantic_embeddings"
    d.mkdir()
    np.save(d / "title_semantic_embeddings-x.npy", np.zeros((3, 16), dtype=np.float32))
    np.save(d / "content_semantic_embeddings-x.npy", np.zeros((3, 16), dtype=np.float32))
    title, content = construct_SAG.read_embeddings(str(tmp_path), "full", "x", 3)
    assert title.shape == content.shape == (3, 16)
    with pytest.raises(ValueError, match=r"title_semantic_embeddings-x\.npy: 3 rows, news_meta gives 4"):
        construct_SAG.read_embeddings(str(tmp_path), "full", "x", 4)
    with pytest.raises(FileNotFoundError):
        construct_SAG.read_embeddings(str(tmp_path), "corpus", "x", 3)


def test_meta_command_writes_the_references_news_meta_files(tmp_path):
    from digat_amd import construct_SAG
    from sag_common import FIXTURE
    construct_SAG.main(["meta", "--data_root", FIXTURE, "--embedding_root", str(tmp_path), "--dataset", "small"])
    for category in categories_with_corpus("small"):
        for mode, sub in construct_SAG.EMBEDDING_DIRS.items():
            with open(tmp_path / sub / ("news_meta-%s.json" % category), encoding="utf-8") as f:
                assert json.load(f) == minted_json("small/%s/meta_%s" % (category, mode))
    assert not os.path.exists(tmp_path / "semantic_embeddings" / "news_meta-weather.json")


def test_header_declares_the_lists_entry_and_the_signature_table_matches():
    from digat_amd import _lib, build
    build.build(verbose=False)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "digat_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(digat_[a-z0-9_]+)\s*\(", text))
    assert {"digat_sag_similar_lists", "digat_sag_similar_lists_workspace_bytes"} <= declared
    assert declared == set(_lib.EXPORTED)
    L = _lib.lib()
    assert L.digat_version() == _lib.ABI_VERSION == 4                                          # an added export: the version stays
    res, args = _lib._SIGNATURES["digat_sag_similar_lists"]
    assert len(args) == 19 and hasattr(L, "digat_sag_similar_lists")
    proto = re.search(r"int digat_sag_similar_lists\((.*?)\);", text, flags=re.S).group(1)
    assert len(proto.split(",")) == 19
    assert L.digat_sag_similar_lists_workspace_bytes(300, 200, 32) == L.digat_sag_cos_topk_workspace_bytes(300, 200, 32) > 0
    # argument checks answer before anything is launched: null pointers, k > 32, dim % 16, an empty corpus, a small workspace
    one = 1 << 20
    call = lambda n, m, dim, top_M, ws: L.digat_sag_similar_lists(*([one, one, n, one, one, m, dim, top_M] + [one] * 7 + [10, one, ws, None]))
    assert L.digat_sag_similar_lists(*([None, one, 4, one, one, 8, 16, 5] + [one] * 7 + [10, one, 1 << 30, None])) == 1
    assert call(4, 0, 16, 5, 1 << 30) == 1 and call(4, 64, 16, 32, 1 << 30) == 2 and call(4, 64, 24, 5, 1 << 30) == 2
    assert call(4, 64, 16, 5, 16) == 3


def test_csr_validation_raises_before_anything_reaches_the_device():
    from digat_amd import construct_SAG
    ok = dict(start=np.array([0, 2, 3], dtype=np.int32), member=np.array([4, 5, 6], dtype=np.int32))
    construct_SAG.validate_csr(ok["start"], ok["member"], 2, 7, "t")
    bad = [(np.array([0, 3, 2], dtype=np.int32), ok["member"], 7),          # a start table that runs backwards
           (ok["start"], np.array([4, 5, 7], dtype=np.int32), 7),          # a member row >= news_num
           (ok["start"], np.array([0, 5, 6], dtype=np.int32), 7),          # the padding row
           (ok["start"], np.array([4, -1, 6], dtype=np.int32), 7),
           (ok["start"], np.array([4, 5, 5], dtype=np.int32), 7),          # two writers for one news row
           (np.array([1, 2, 3], dtype=np.int32), ok["member"], 7), (np.array([0, 2, 4], dtype=np.int32), ok["member"], 7),
           (np.array([0, 3], dtype=np.int32), ok["member"], 7)]
    for start, member, news_num in bad:
        with pytest.raises(ValueError):
            construct_SAG.validate_csr(start, member, 2, news_num, "t")
    with pytest.raises(ValueError, match="empty group"):
        construct_SAG.validate_csr(np.array([0, 0, 3], dtype=np.int32), ok["member"], 2, 7, "t", nonempty=True)
    # ... and the device mirror validates first: with CPU tensors a bad table is still the ValueError, not the no-CPU-path error
    x = torch.zeros(2, 16)
    for start, member, news_num in bad[:2]:
        with pytest.raises(ValueError):
            construct_SAG.similar_news_lists_device(x, x, x, x, 3, start, member, ok["start"], ok["member"], news_num)
        with pytest.raises(ValueError):
            construct_SAG.similar_news_lists_device(x, x, x, x, 3, ok["start"], ok["member"], start, member, news_num)
