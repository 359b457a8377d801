"""Shared by the SAG-from-embeddings suites: the ``sag_tiny`` fixture (tools/make_sag_fixture.py), what the reference made of it
(tests/golden/sag_tiny_golden.npz, tools/mint_sag_golden.py) and the loader's arguments for it."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "sag_tiny")
DATASETS = ("small", "large")                       # the reference's dataset_type: 'small' keeps test news out of the corpus side
TOP_M, HOPS = 5, 2
LOAD = dict(max_history_num=10, max_title_length=8, word_threshold=1, sag_neighbors=TOP_M, sag_hops=HOPS, word_embedding_dim=20)
_cache = {}


def embedding_root(dataset):
    return os.path.join(FIXTURE, dataset + "-SAG")


def minted():
    if "g" not in _cache:
        with np.load(os.path.join(GOLDEN, "sag_tiny_golden.npz"), allow_pickle=False) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def minted_json(key):
    return json.loads(str(minted()[key]))


def corpus_inputs():
    """(``mind.read_news_text``'s list, the loader's dictionaries) of the fixture; one parse, shared and left unchanged."""
    from digat_amd import mind
    if "inputs" not in _cache:
        roots = [os.path.join(FIXTURE, s) for s in mind.SPLITS]
        dictionaries = mind.build_dictionaries(mind.read_news(roots), roots[0], LOAD["word_threshold"])
        assert dictionaries["news_ID"] == minted_json("news_ID") and dictionaries["category"] == minted_json("category")
        _cache["inputs"] = (mind.read_news_text(roots), dictionaries)
    return _cache["inputs"]


def categories_with_corpus(dataset):
    return [c for c in minted_json("category") if "%s/%s/avg_values" % (dataset, c) in minted()]
