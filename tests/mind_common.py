"""Shared by the MIND loader suites: the tiny fixture, what the reference made of it, and the loader's arguments for it."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "mind_tiny")
SIMILARITY = os.path.join(FIXTURE, "similarity-3.json")
# the shapes tools/mint_mind_golden.py ran the reference with (devset_tiny's): H = 10, Lw = 8, M = 3, one hop
LOAD = dict(max_history_num=10, max_title_length=8, word_threshold=3, sag_neighbors=3, sag_hops=1, word_embedding_dim=20)
DICTS = (("user_ID", "user_ID"), ("news_ID", "news_ID"), ("category", "category"), ("subCategory", "subCategory"), ("word_dict", "word"))
_cache = {}


def minted():
    if "g" not in _cache:
        with np.load(os.path.join(GOLDEN, "mind_tiny_golden.npz"), allow_pickle=False) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def minted_dict(name):
    return json.loads(str(minted()["dict_" + name]))


def loaded(**kw):
    """The fixture through ``mind.load`` (no artefacts, no similarity file unless named: singleton news graphs); one parse per
    argument set, shared and left unchanged by the tests."""
    from digat_amd import mind
    key = tuple(sorted(kw.items()))
    if key not in _cache:
        _cache[key] = mind.load(FIXTURE, **{**LOAD, **kw}, verbose=False)
    return _cache[key]
