"""CPU suite: the MIND loader (digat_amd/mind.py) against what the reference's ``MIND_Corpus.preprocess`` / ``MIND_Corpus(config)``
made of the same files (tests/golden/mind_tiny, minted by tools/mint_mind_golden.py) — dictionaries, news arrays, the three splits,
the artefact route, the cache — and the two seams around it: ``Config`` without ``--data_root`` and ``Trainer``'s ``dev_dc``."""
import json
import os
import pickle
import shutil
import types

import numpy as np
import pytest
import torch

from mind_common import DICTS, FIXTURE, LOAD, loaded, minted, minted_dict


def test_dictionaries_equal_the_references_in_content_and_order():
    corpus = loaded()
    for ours, theirs in DICTS:
        want = minted_dict(theirs)
        assert list(corpus.dictionaries[ours].items()) == list(want.items()), ours
    words = corpus.dictionaries["word_dict"]
    assert words["<PAD>"] == 0 and words["<UNK>"] == 1 and "<NUM>" in words
    assert "zebra" not in words and "quokka" not in words          # under the threshold; first seen in dev (four times there)
    assert "cafe" not in words and "resume" not in words           # e-acute folded, then under the threshold too
    assert (corpus.user_num, corpus.category_num, corpus.subCategory_num, corpus.vocabulary_size) == \
        tuple(len(minted_dict(n)) for n in ("user_ID", "category", "subCategory", "word"))


def test_news_arrays_equal_the_references():
    corpus, g = loaded(), minted()
    assert corpus.news_title_text.dtype == np.int32 and corpus.news_title_mask.dtype == bool and corpus.news_category.dtype == np.int64
    assert np.array_equal(corpus.news_title_text, g["news_title_text"])
    assert np.array_equal(corpus.news_title_mask, g["news_title_mask"])
    assert np.array_equal(corpus.news_category, g["news_category"])
    assert corpus.news_title_mask.all(axis=1).any()                 # a title longer than Lw was cut
    assert not corpus.news_title_mask[0].any() and not corpus.news_title_text[0].any()


@pytest.mark.parametrize("split", ["train", "dev", "test"])
def test_split_user_side_equals_the_references(split):
    s, g = loaded().splits[split], minted()
    assert s.history.dtype == np.int32 and s.user_category_indices.dtype == np.int64 and s.user_category_mask.dtype == bool
    assert np.array_equal(s.user_category_indices, g[split + "_user_history_category_indices"])
    assert np.array_equal(s.user_category_mask, g[split + "_user_history_category_mask"])
    assert np.array_equal(s.user_graph_mask, g[split + "_user_history_graph_mask"])
    lengths = (s.history != 0).sum(axis=1)
    assert lengths.min() == 0 and lengths.max() == 10               # empty histories; longer ones cut to the last H
    assert s.user_graph is None                                     # the [I, U, U] table is never built on the host
    if split != "train":
        assert np.array_equal(s.row_candidate, g[split + "_candidate"]) and np.array_equal(s.row_impression, g[split + "_indices"])
        assert np.array_equal(s.history[s.row_impression], g[split + "_history"])
    if split == "dev":
        assert np.array_equal(s.row_label, g["dev_label"])


def test_train_rows_reproduce_the_references_behaviours_but_the_skipped_ones():
    from digat_amd.train_input import behavior_arrays
    s, g = loaded().train, minted()
    imp, click, off, pool = behavior_arrays(s)
    skipped = g["train_skipped"]
    assert len(skipped) == 2                                        # the two clicks of the impression without a non-clicked news
    keep = np.setdiff1d(np.arange(len(g["train_click"])), skipped)
    assert np.array_equal(click, g["train_click"][keep]) and np.array_equal(imp, g["train_behavior_index"][keep])
    assert np.array_equal(s.history[imp], g["train_history"][keep])
    want_off = g["train_pool_offsets"]
    assert [pool[a:b].tolist() for a, b in zip(off[:-1], off[1:])] == [g["train_pool"][want_off[k]:want_off[k + 1]].tolist() for k in keep]
    assert np.bincount(imp).max() == 3                              # several clicks in one impression


def test_unlabelled_test_file_parses_to_the_same_rows_without_labels(tmp_path):
    from digat_amd import mind
    root = tmp_path / "data"
    shutil.copytree(FIXTURE, root)
    shutil.copy(os.path.join(FIXTURE, "test_unlabelled", "behaviors.tsv"), root / "test" / "behaviors.tsv")
    labelled, bare = loaded().test, mind.load(str(root), **LOAD, verbose=False).test
    assert bare.row_label is None and labelled.row_label is not None and labelled.row_label.dtype == np.int8
    for name in ("history", "user_category_indices", "user_category_mask", "row_impression", "row_candidate"):
        assert np.array_equal(getattr(bare, name), getattr(labelled, name)), name


def write_artefacts(root, dataset="MIND-small"):
    """The minted arrays in the reference's file names and formats (MIND_corpus.py:25-32)."""
    g = minted()
    os.makedirs(root, exist_ok=True)
    for name in ("user_ID", "news_ID", "category", "subCategory"):
        with open(os.path.join(root, f"{name}-{dataset}.json"), "w", encoding="utf-8") as f:
            json.dump(minted_dict(name), f)
    with open(os.path.join(root, f"vocabulary-3-8-{dataset}.json"), "w", encoding="utf-8") as f:
        json.dump(minted_dict("word"), f)
    with open(os.path.join(root, f"word_embedding-3-20-8-{dataset}.pkl"), "wb") as f:
        pickle.dump(torch.from_numpy(g["word_embedding"]), f)
    mask = g["news_graph_mask"].copy()
    mask[:, 0] = True                                               # as preprocess writes it; the loader clears the column (:210)
    with open(os.path.join(root, f"news_graph-1-3-{dataset}.pkl"), "wb") as f:
        pickle.dump({"news_node_ID": g["news_node_ID"], "news_graph": g["news_graph"], "news_graph_mask": mask}, f, protocol=4)
    with open(os.path.join(root, f"user_history_graph-10-{dataset}.pkl"), "wb") as f:
        pickle.dump({f"{s}_user_history_{p}": g[f"{s}_user_history_{p}"] for s in ("train", "dev", "test")
                     for p in ("graph", "graph_mask", "category_mask", "category_indices")}, f, protocol=4)


def test_artefact_route_returns_the_same_corpus(tmp_path):
    from digat_amd import mind
    g, plain = minted(), loaded()
    art = str(tmp_path / "artefacts")
    write_artefacts(art)
    corpus = mind.load(FIXTURE, **LOAD, artefact_root=art, verbose=False)
    assert corpus.dictionaries == plain.dictionaries
    for name in ("news_title_text", "news_title_mask", "news_category"):
        assert np.array_equal(getattr(corpus, name), getattr(plain, name)), name
    for split in ("train", "dev", "test"):
        for name in ("history", "user_category_indices", "user_category_mask", "row_impression", "row_candidate", "row_label"):
            assert np.array_equal(getattr(corpus.splits[split], name), getattr(plain.splits[split], name)), (split, name)
    assert corpus.news_graph_source == "artefact"
    assert np.array_equal(corpus.news_node_ID, g["news_node_ID"]) and np.array_equal(corpus.news_graph, g["news_graph"])
    assert np.array_equal(corpus.news_graph_mask, g["news_graph_mask"]) and not corpus.news_graph_mask[:, 0].any()
    assert np.array_equal(corpus.word_embedding, g["word_embedding"]) and corpus.word_embedding.dtype == np.float32
    # the dictionaries are USED, not rebuilt: a vocabulary in another order gives other token ids
    words = minted_dict("word")
    swapped = {**words, "the": words["a"], "a": words["the"]}
    with open(os.path.join(art, "vocabulary-3-8-MIND-small.json"), "w", encoding="utf-8") as f:
        json.dump(swapped, f)
    other = mind.load(FIXTURE, **LOAD, artefact_root=art, verbose=False)
    assert not np.array_equal(other.news_title_text, plain.news_title_text)
    assert np.array_equal(other.news_title_text == words["a"], plain.news_title_text == words["the"])


def test_artefact_route_refuses_inconsistent_artefacts(tmp_path):
    from digat_amd import mind
    art = str(tmp_path / "artefacts")
    write_artefacts(art)
    # the user-graph artefact: only its category indices are read, and they must be the loader's
    path = os.path.join(art, "user_history_graph-10-MIND-small.pkl")
    with open(path, "rb") as f:
        u = pickle.load(f)
    u["dev_user_history_category_indices"] = u["dev_user_history_category_indices"].copy()
    u["dev_user_history_category_indices"][0, 0] ^= 1
    with open(path, "wb") as f:
        pickle.dump(u, f, protocol=4)
    with pytest.raises(ValueError, match="category indices"):
        mind.load(FIXTURE, **LOAD, artefact_root=art, verbose=False)
    os.remove(path)
    # a news_ID dictionary with one news removed: the reference's count check (:251)
    ids = minted_dict("news_ID")
    ids.pop(list(ids)[-1])
    with open(os.path.join(art, "news_ID-MIND-small.json"), "w", encoding="utf-8") as f:
        json.dump(ids, f)
    with pytest.raises(ValueError, match="news num mismatch"):
        mind.load(FIXTURE, **LOAD, artefact_root=art, verbose=False)


def test_singleton_graphs_and_number_under_the_threshold():
    from digat_amd import mind
    corpus = loaded()
    node_ID, graph, mask = corpus.graphs()
    assert corpus.news_graph_source == "singleton" and node_ID.shape == (corpus.news_num, 4) and node_ID.dtype == np.int32
    assert np.array_equal(node_ID[:, 0], np.arange(corpus.news_num)) and not node_ID[:, 1:].any() and not mask.any()
    assert np.array_equal(graph, np.broadcast_to(np.eye(4, dtype=bool), graph.shape))
    # a threshold no word reaches: <NUM> is absent from the vocabulary, and numbers read as <UNK> where the reference raises
    bare = mind.load(FIXTURE, **{**LOAD, "word_threshold": 10 ** 6}, verbose=False)
    assert bare.dictionaries["word_dict"] == {"<PAD>": 0, "<UNK>": 1}
    assert np.array_equal(bare.news_title_text, bare.news_title_mask.astype(np.int32))


def equal_corpora(a, b):
    assert a.dictionaries == b.dictionaries and [list(d.items()) for d in a.dictionaries.values()] == [list(d.items()) for d in b.dictionaries.values()]
    for name in ("news_title_text", "news_title_mask", "news_category", "news_subCategory", "news_node_ID", "news_graph", "news_graph_mask"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    for split in ("train", "dev", "test"):
        for name in ("history", "user_category_indices", "user_category_mask", "row_impression", "row_candidate", "row_label"):
            x, y = getattr(a.splits[split], name), getattr(b.splits[split], name)
            assert x.dtype == y.dtype and np.array_equal(x, y), (split, name)


def test_cache_round_trips_and_a_stale_one_is_rebuilt(tmp_path, monkeypatch):
    from digat_amd import mind
    root, cache = tmp_path / "data", str(tmp_path / "cache")
    shutil.copytree(FIXTURE, root)
    first = mind.load(str(root), **LOAD, data_cache=cache, verbose=False)
    assert sorted(os.listdir(cache)) == ["dev.npz", "dictionaries.json", "header.json", "news.npz", "test.npz", "train.npz"]
    with monkeypatch.context() as m:                                # the second load reads no TSV
        m.setattr(mind, "read_news", lambda roots: pytest.fail("the cache was not used"))
        again = mind.load(str(root), **LOAD, data_cache=cache, verbose=False)
    equal_corpora(first, again)
    equal_corpora(again, mind.MindCorpus.load(cache))
    # other parameters: rebuilt, not trusted
    shorter = mind.load(str(root), **{**LOAD, "max_history_num": 6}, data_cache=cache, verbose=False)
    assert shorter.dev.history.shape[1] == 6 and mind.MindCorpus.load(cache).dev.history.shape[1] == 6
    mind.load(str(root), **LOAD, data_cache=cache, verbose=False)
    # a TSV whose size changed: rebuilt
    with open(root / "dev" / "behaviors.tsv", "r", encoding="utf-8") as f:
        line = f.readline()
    with open(root / "dev" / "behaviors.tsv", "a", encoding="utf-8") as f:
        f.write(line)
    grown = mind.load(str(root), **LOAD, data_cache=cache, verbose=False)
    assert grown.dev.history.shape[0] == first.dev.history.shape[0] + 1
    assert mind.MindCorpus.load(cache).dev.history.shape[0] == first.dev.history.shape[0] + 1


# Config([]) as it was before the MIND flags existed
CONFIG_DEFAULTS = {
    'MSA_head_dim': 25, 'MSA_head_num': 16, 'SAG_hops': 2, 'SAG_neighbors': 5, 'attention_dim': 256, 'batch_size': 64, 'category_num': 17,
    'cnn_kernel_num': 400, 'cnn_method': 'naive', 'cnn_window_size': 3, 'dataset': 'MIND-small', 'dev_criterion': 'avg',
    'dev_model_path': 'best_model/MIND-small/MSA-DIGAT/#1/MSA-DIGAT', 'dropout_rate': 0.2, 'early_stopping_epoch': 5, 'epoch': 16,
    'gradient_clip_norm': 1, 'graph_depth': 3, 'graph_encoder': 'DIGAT', 'inference_projection': 'auto', 'local_rank': -1, 'lr': 0.0001,
    'max_history_num': 50, 'max_steps': 0, 'max_title_length': 1, 'mode': 'train', 'negative_sample_num': 4, 'news_embedding_dim': 400,
    'news_encoder': 'MSA', 'news_graph_size': 26, 'recommend_k': 10, 'recommend_output': '', 'seed': 0, 'synthetic_impressions': 2048,
    'synthetic_news': 8192, 'test_model_path': 'best_model/MIND-small/MSA-DIGAT/#1/MSA-DIGAT', 'test_output_file': '',
    'train_input': 'host', 'train_precision': 'fp32', 'user_graphs': 'table', 'weight_decay': 0, 'word_embedding_dim': 300}
NOT_PARSED = ('category_num', 'news_graph_size', 'max_title_length')


def test_config_without_data_root_is_todays(monkeypatch):
    from digat_amd.config import Config
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    have = dict(vars(Config([])))
    assert have.pop("attribute_dict") == {k: v for k, v in CONFIG_DEFAULTS.items() if k not in NOT_PARSED}
    assert have == CONFIG_DEFAULTS
    # with it: the loader's flags are attributes, the title length is the reference's, and the corpus decides the sizes
    c = Config(["--data_root", FIXTURE, "--similarity_file", "s.json", "--model_dir", "m"])
    assert (c.data_root, c.similarity_file, c.model_dir, c.artefact_root, c.word_embedding_file, c.data_cache) == (FIXTURE, "s.json", "m", "", "", "")
    assert (c.word_threshold, c.max_title_length) == (3, 32)
    c.set_corpus(loaded())
    assert (c.category_num, c.vocabulary_size, c.user_num, c.subCategory_num) == (5, 39, 22, 8)
    assert Config(["--model_dir", "m"]).model_dir == "m" and not hasattr(Config([]), "model_dir")


def test_trainer_scores_dev_dc_when_given(monkeypatch):
    """The harness of tests/test_trainer_cpu.py: ``evaluate_dev`` is handed ``dev_dc`` when there is one, else the training corpus."""
    from digat_amd import synthetic, trainer as T
    from digat_amd.model import Model, PrecomputedNewsEncoder
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=4, max_history_num=10, category_num=5,
                                graph_depth=1, dropout_rate=0.2, epoch=2, batch_size=4, lr=1e-3, early_stopping_epoch=2, dev_criterion="auc")
    corpus = synthetic.make_corpus(synthetic.SynthSpec(news_num=64, sag_neighbors=3, sag_hops=1, max_history_num=10, category_num=5,
                                                       embedding_dim=64, impressions=12, mean_candidates=6.0, max_candidates=12, seed=4))
    train_dc, dev_dc = types.SimpleNamespace(news_embedding=torch.zeros(1)), types.SimpleNamespace(news_embedding=torch.zeros(1))
    for given, want in ((dev_dc, dev_dc), (None, train_dc)):
        model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.zeros(16, 64), trainable=True))
        tr = T.Trainer(model, cfg, train_dc, T.SyntheticTrainSet(corpus, 4, 0), dev_labels=corpus.row_label, dev_dc=given)
        seen = []

        def fake_dev(net, dc_, labels, bs, as_tuple=False):
            seen.append(dc_)
            return (0.5, 0.3, 0.3, 0.3)
        monkeypatch.setattr(tr, "train_step", lambda idx, read_loss=True: 0.0 if read_loss else torch.zeros(()))
        monkeypatch.setattr(tr, "batches", lambda e: iter([np.arange(2)]))
        monkeypatch.setattr(T, "evaluate_dev", fake_dev)
        tr.train()
        assert len(seen) == 2 and all(s is want for s in seen)


def test_second_split_shares_the_first_ones_news_tensors_on_the_host():
    """``news_from`` without a GPU (derived user graphs: nothing runs on a device): no second copy of any news tensor."""
    from digat_amd import util
    corpus = loaded()
    a = util.DeviceCorpus.from_numpy(corpus.train, torch.device("cpu"), user_graphs="derived")
    b = util.DeviceCorpus.from_numpy(corpus.dev, torch.device("cpu"), user_graphs="derived", news_from=a)
    assert a.title_text.dtype == torch.int32 and a.title_mask.dtype == torch.bool and tuple(a.news_embedding.shape) == (corpus.news_num, 0)
    for name in ("news_node_ID", "news_graph", "news_graph_mask", "title_text", "title_mask", "news_embedding"):
        assert getattr(a, name) is getattr(b, name), name
    assert b.news_source is a and b.category_num == 5 and b.user_graph is None
    assert b.history.shape[0] == 24 and a.history.shape[0] == 40 and b.rows == corpus.dev.rows
