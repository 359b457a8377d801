#!/usr/bin/env python3
"""Write ``tests/golden/sag_tiny/``: a tiny MIND-shaped corpus with sentence embeddings, for the embeddings -> similar-news lists
-> news graphs chain (``construct_SAG.build_similarity``, ``mind.load(semantic_embedding_root=...)``).

Three ``news.tsv`` / ``behaviors.tsv`` pairs (train, dev, test) and, for the reference's two dataset types, seeded ``.npy``
embeddings (dim 32) per category and mode in the reference's layout:
``<small|large>-SAG/{semantic_embeddings,corpus_semantic_embeddings}/{title,content}_semantic_embeddings-<category>.npy``.
An embedding is a function of its TEXT alone (a sum of seeded word vectors plus seeded per-text noise, normalised), so one text has
one embedding in every mode and dataset type, as a sentence model would give it.

What the corpus holds on purpose:
  * duplicate titles within a category, inside train and across train and test (one title group, several news);
  * a news with an empty title, one with an empty abstract, one with both empty (no text at all: random neighbours);
  * duplicated abstracts under different titles (the content gets the title in front);
  * ``weather``: a category present only in test (no corpus: skipped, empty lists);
  * ``solo``: one corpus group on the small dataset (M' = 0: the stop test that never fires), two on the large one;
  * ``few``: fewer than top_M + 1 corpus groups;
  * upper case and ``é`` in titles.
The texts to embed come from ``construct_SAG.news_meta``; ``tools/mint_sag_golden.py`` then holds that function, and everything
after it, to the reference.

Usage:  python tools/make_sag_fixture.py [--seed N]
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "sag_tiny")
DIM, TOP_M = 32, 5
SEED = 8          # tools/mint_sag_golden.py asserts the separation of the cosines this seed gives

POOLS = {
    "sports": "match goal team coach league season striker final cup transfer injury stadium".split(),
    "finance": "market stock bank rate profit shares bond inflation merger fund".split(),
    "weather": "storm rain heat flood wind snow frost".split(),
    "solo": "chess opening gambit endgame rook bishop".split(),
    "few": "recipe oven bread butter salt sugar".split(),
}


def sentence(rng, pool, words):
    return " ".join(rng.choice(pool, size=words, replace=False))


def make_news(rng):
    """{split: [(news_ID, category, title, abstract)]}; ids N1.. in file order."""
    out = {"train": [], "dev": [], "test": []}
    serial = [0]

    def add(split, category, title, abstract):
        serial[0] += 1
        out[split].append(("N%d" % serial[0], category, title, abstract))
        return out[split][-1]

    def plain(split, category, count):
        for _ in range(count):
            add(split, category, sentence(rng, POOLS[category], 4).capitalize(), sentence(rng, POOLS[category], 6))

    sp = POOLS["sports"]
    plain("train", "sports", 5)
    twice = add("train", "sports", "Derby Fiancé final goal", sentence(rng, sp, 6))
    add("train", "sports", twice[2], sentence(rng, sp, 6))                      # the same title inside train
    shared = sentence(rng, sp, 6)
    add("train", "sports", sentence(rng, sp, 4), shared)                        # duplicated abstracts, two titles
    add("train", "sports", sentence(rng, sp, 4), shared)
    add("train", "sports", "", sentence(rng, sp, 6))                            # empty title
    add("train", "sports", sentence(rng, sp, 4), "")                            # empty abstract
    add("train", "sports", "", "")                                              # no text
    plain("train", "finance", 5)
    again = add("train", "finance", sentence(rng, POOLS["finance"], 4), sentence(rng, POOLS["finance"], 6))
    one = add("train", "solo", "Queen gambit opening", sentence(rng, POOLS["solo"], 3))
    add("train", "solo", one[2], "")                                            # one title group is the whole corpus
    plain("train", "few", 2)
    plain("dev", "sports", 4)
    plain("dev", "finance", 3)
    plain("dev", "few", 1)
    plain("test", "sports", 3)
    add("test", "sports", twice[2].upper(), sentence(rng, sp, 6))               # the train title again, in test
    add("test", "sports", "", "")
    plain("test", "finance", 2)
    add("test", "finance", again[2], "")
    plain("test", "weather", 2)
    add("test", "solo", "Endgame chess", sentence(rng, POOLS["solo"], 3))
    plain("test", "few", 1)
    return out


def make_behaviors(rng, news):
    """A few impressions per split over the news that have a title (``behaviors.tsv``: id, user, time, history, impressions)."""
    titled = {s: [n[0] for n in rows if n[2]] for s, rows in news.items()}
    out = {}
    for split, count in (("train", 16), ("dev", 8), ("test", 8)):
        known = titled["train"] + (titled[split] if split != "train" else [])
        lines = []
        for i in range(count):
            history = rng.choice(titled["train"], size=int(rng.integers(0, 7)), replace=False)
            cands = list(rng.choice(known, size=int(rng.integers(3, 7)), replace=False))
            labels = [1] + [0] * (len(cands) - 1)
            lines.append("%d\tU%d\t11/11/2019 9:00:00 AM\t%s\t%s" % (i + 1, int(rng.integers(1, 7)), " ".join(history),
                                                                    " ".join("%s-%d" % (c, l) for c, l in zip(cands, labels))))
        out[split] = lines
    return out


class TextEmbedder:
    """text -> unit vector: the sum of its words' seeded vectors plus seeded per-text noise; one vector per distinct text."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.words, self.texts = {}, {}

    def __call__(self, text):
        if text not in self.texts:
            total = np.zeros(DIM)
            for w in text.split(" "):
                if w not in self.words:
                    self.words[w] = self.rng.standard_normal(DIM)
                total += self.words[w]
            total = total / np.sqrt(len(text.split(" "))) + 0.35 * self.rng.standard_normal(DIM)
            self.texts[text] = (total / np.linalg.norm(total) * self.rng.uniform(0.5, 2.0)).astype(np.float32)
        return self.texts[text]


def main():
    from digat_amd import construct_SAG, mind
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=SEED)
    seed = ap.parse_args().seed
    rng = np.random.default_rng(seed)
    news = make_news(rng)
    behaviors = make_behaviors(rng, news)
    shutil.rmtree(OUT, ignore_errors=True)
    for split in mind.SPLITS:
        os.makedirs(os.path.join(OUT, split))
        with open(os.path.join(OUT, split, "news.tsv"), "w", encoding="utf-8") as f:
            for news_ID, category, title, abstract in news[split]:
                f.write("\t".join([news_ID, category, category + "-sub", title, abstract, "https://example.invalid/" + news_ID, "[]", "[]"]) + "\n")
        with open(os.path.join(OUT, split, "behaviors.tsv"), "w", encoding="utf-8") as f:
            f.write("\n".join(behaviors[split]) + "\n")
    embed = TextEmbedder(seed + 1)
    rows, has_corpus = construct_SAG.category_rows(mind.read_news_text([os.path.join(OUT, s) for s in mind.SPLITS]))
    files = 0
    for dataset in ("small", "large"):
        for category in rows:
            if category not in has_corpus:
                continue
            for mode, sub in construct_SAG.EMBEDDING_DIRS.items():
                _, _, titles, contents, _ = construct_SAG.news_meta(rows[category], mode, construct_SAG.excludes_test(dataset))
                d = os.path.join(OUT, dataset + "-SAG", sub)
                os.makedirs(d, exist_ok=True)
                for kind, texts in (("title", titles), ("content", contents)):
                    np.save(os.path.join(d, "%s_semantic_embeddings-%s.npy" % (kind, category)), np.stack([embed(t) for t in texts]))
                    files += 1
    with open(os.path.join(OUT, "README.md"), "w", encoding="utf-8") as f:
        f.write("Written by `tools/make_sag_fixture.py --seed %d` (top_M %d, dim %d); what the reference makes of it is in\n"
                "`../sag_tiny_golden.npz` (`tools/mint_sag_golden.py`).  Data only.\n" % (seed, TOP_M, DIM))
    print("wrote %s: %d news, %d embedding files" % (os.path.relpath(OUT, REPO), sum(len(v) for v in news.values()), files))


if __name__ == "__main__":
    main()
