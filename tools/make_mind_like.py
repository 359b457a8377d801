#!/usr/bin/env python3
"""Write MIND-format files from ``synthetic.make_corpus`` at a requested scale: something for ``mind.load`` and
``python -m digat_amd.main --data_root`` to be timed on where MIND itself is not at hand.

``<out>/{train,dev,test}/{news,behaviors}.tsv`` and ``<out>/similarity-<M>.json``.  The three splits list the same news; each has its
own impressions (histories, candidates and labels of a synthetic corpus of that many impressions).  Titles are Zipf-distributed
words of a made-up vocabulary, 4-18 per title, with the odd number, capital and punctuation mark.  The defaults are MIND-small's
dev scale: 65 238 news and 73 152 dev impressions.

Usage:  python tools/make_mind_like.py OUT [--news 65238] [--dev_impressions 73152] [--train_impressions 8192]
                                           [--test_impressions 2048] [--sag_neighbors 5] [--seed 0]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from digat_amd import synthetic  # noqa: E402


def titles(rng, count: int, vocabulary: int = 30000):
    words = np.array(["w%d" % i for i in range(vocabulary)], dtype=object)
    length = rng.integers(4, 19, size=count)
    ids = np.minimum(rng.zipf(1.3, size=int(length.sum())) - 1, vocabulary - 1)
    out, at = [], 0
    for k, n in enumerate(length):
        w = list(words[ids[at:at + n]])
        at += n
        if k % 5 == 0:
            w[0] = str(int(ids[at - 1]) % 100)
        if k % 3 == 0:
            w[-1] = w[-1].capitalize() + "!"
        out.append(" ".join(w))
    return out


def write_split(root: str, news_lines, corpus, name_of):
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "news.tsv"), "w", encoding="utf-8") as f:
        f.writelines(news_lines)
    bounds = np.r_[0, np.flatnonzero(np.diff(corpus.row_impression)) + 1, corpus.rows]
    tokens = [name_of[c] + ("-1" if l else "-0") for c, l in zip(corpus.row_candidate.tolist(), corpus.row_label.tolist())]
    with open(os.path.join(root, "behaviors.tsv"), "w", encoding="utf-8") as f:
        for i, (s, e) in enumerate(zip(bounds[:-1], bounds[1:])):
            history = " ".join(name_of[h] for h in corpus.history[i].tolist() if h)
            f.write("%d\tU%d\t11/13/2019 8:36:57 AM\t%s\t%s\n" % (i + 1, i % 50000, history, " ".join(tokens[s:e])))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("out")
    p.add_argument("--news", type=int, default=65238)
    p.add_argument("--train_impressions", type=int, default=8192)
    p.add_argument("--dev_impressions", type=int, default=73152)
    p.add_argument("--test_impressions", type=int, default=2048)
    p.add_argument("--sag_neighbors", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args(argv)
    rng = np.random.default_rng(a.seed)
    news_num = a.news + 1                                                        # row 0 is <PAD>
    name_of = ["<PAD>"] + ["N%d" % i for i in range(1, news_num)]
    lines, category = None, None
    for k, (split, impressions) in enumerate((("train", a.train_impressions), ("dev", a.dev_impressions), ("test", a.test_impressions))):
        # the corpus's own news graphs are not written (the similarity file below is): the cheapest SAG setting
        corpus = synthetic.make_corpus(synthetic.SynthSpec(news_num=news_num, sag_neighbors=1, sag_hops=1, embedding_dim=4,
                                                           impressions=impressions, seed=a.seed + k))
        if lines is None:                                                        # one news side for the three splits: the first's
            category = corpus.news_category
            lines = ["%s\tcat%d\tsub%d\t%s\t\t\t[]\t[]\n" % (name_of[i], category[i], category[i] * 4 + i % 4, t)
                     for i, t in zip(range(1, news_num), titles(rng, news_num - 1))]
        write_split(os.path.join(a.out, split), lines, corpus, name_of)
        print("%s: %d impressions, %d rows" % (split, impressions, corpus.rows), flush=True)
    ids, cos, length = synthetic.make_similarity_lists(rng, news_num, a.sag_neighbors, 0.02)
    sim = {name_of[i]: [[name_of[int(ids[i, e])], float(cos[i, e])] for e in range(int(length[i]))] for i in range(news_num)}
    with open(os.path.join(a.out, "similarity-%d.json" % a.sag_neighbors), "w", encoding="utf-8") as f:
        json.dump(sim, f)


if __name__ == "__main__":
    main()
