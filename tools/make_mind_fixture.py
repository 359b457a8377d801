#!/usr/bin/env python3
"""Write the tiny MIND-format fixture ``tests/golden/mind_tiny`` (seeded; a few KB of data).

Layout: ``{train,dev,test}/{news,behaviors}.tsv`` in the MIND column order (news: id, category, subcategory, title, abstract,
url, title entities, abstract entities; behaviours: impression id, user id, time, history, impressions), ``similarity-3.json``
in the format of the reference's ``similarity-M.json`` (``{news_ID: [[news_ID, cos], ...]}``, every news a key, ``<PAD>`` too)
and ``test_unlabelled/behaviors.tsv``: the test behaviours without their ``-0/-1`` suffixes (MIND-large's test file).

Shapes as ``devset_tiny``: 5 categories, about 60 news over the three files, made for H = 10, Lw = 8, M = 3, one hop (N = 4).
The cases a loader can get wrong are planted by hand below and asserted at the end.

Usage:  python tools/make_mind_fixture.py [output directory]
"""
from __future__ import annotations

import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATEGORIES = {"news": ["newsus", "newsworld"], "sports": ["football_nfl", "golf"], "finance": ["markets"],
              "lifestyle": ["lifestyleroyals", "lifestylebuzz"], "health": ["wellness"]}
COMMON = ("the a of in to for and on with new says after over from at how why what this that his her year day home "
          "team city market plan game win deal report star").split()

# planted titles: upper case, punctuation, numbers, e-acute, a title longer than Lw = 8, a word under the threshold ("zebra", once),
# float()'s idea of a number ("nan", "1_000"), and — in PLANTED_DEV — a word that first appears in dev ("quokka": never counted)
PLANTED_TRAIN = [
    "Café Opens In Paris, 2019!",
    "The 50 Best Deals Of The Year; Why 3 Of 4 Buyers Say This One Wins",
    "A zebra walks into the market",
    "Résumé tips: how to win in 2020?",
    "Team wins 3.5 million | city says nan",
    "What 1_000 fans say",
]
PLANTED_DEV = ["The quokka plan", "Why the quokka wins", "A quokka in the city", "Quokka, quokka!"]


def title(rng: random.Random) -> str:
    words = [rng.choice(COMMON) for _ in range(rng.randint(3, 7))]
    if rng.random() < 0.3:
        words[rng.randrange(len(words))] = str(rng.randint(1, 99))
    text = " ".join(words)
    if rng.random() < 0.5:
        text = text.capitalize()
    if rng.random() < 0.3:
        text += rng.choice(".!?")
    return text


def news_line(nid: str, rng: random.Random, text: str) -> str:
    cat = rng.choice(sorted(CATEGORIES))
    sub = rng.choice(CATEGORIES[cat])
    return "\t".join([nid, cat, sub, text, "Abstract of " + nid + ".", "https://example.invalid/" + nid + ".html", "[]", "[]"]) + "\n"


def behaviours(rng: random.Random, count: int, first_id: int, users, news_ids, histories, forced=()):
    """``count`` behaviour lines.  ``histories``: history lengths to cycle through; ``forced``: impressions fields planted verbatim."""
    lines = []
    for k in range(count):
        hist_len = histories[k % len(histories)]
        history = " ".join(rng.choice(news_ids) for _ in range(hist_len))
        if k < len(forced):
            imps = forced[k]
        else:
            cands = rng.sample(news_ids, rng.randint(2, 7))
            clicks = set(rng.sample(range(len(cands)), 1 if rng.random() < 0.7 else min(2, len(cands) - 1)))
            imps = " ".join(c + ("-1" if i in clicks else "-0") for i, c in enumerate(cands))
        lines.append("\t".join([str(first_id + k), rng.choice(users), "11/13/2019 8:36:57 AM", history, imps]) + "\n")
    return lines


def main(out=None):
    out = out or os.path.join(REPO, "tests", "golden", "mind_tiny")
    rng = random.Random(20191113)
    ids = ["N%d" % (1000 + 7 * i) for i in range(60)]
    train_ids, dev_only, test_only = ids[:36], ids[36:48], ids[48:60]
    lines = {}
    for k, nid in enumerate(train_ids):
        lines[nid] = news_line(nid, rng, PLANTED_TRAIN[k] if k < len(PLANTED_TRAIN) else title(rng))
    for k, nid in enumerate(dev_only):
        lines[nid] = news_line(nid, rng, PLANTED_DEV[k] if k < len(PLANTED_DEV) else title(rng))
    for nid in test_only:
        lines[nid] = news_line(nid, rng, title(rng))
    # news repeated across splits: dev and test files repeat a part of the training news and add their own
    split_news = {"train": train_ids, "dev": train_ids[4:24] + dev_only, "test": dev_only[:4] + train_ids[12:30] + test_only}
    users = ["U%d" % (100 + i) for i in range(25)]
    hist = [3, 0, 7, 14, 1, 10, 0, 5, 11, 2, 9]              # empty histories, and histories longer than H = 10
    t = split_news["train"]
    forced_train = [" ".join([t[0] + "-1", t[5] + "-0", t[9] + "-1", t[2] + "-1", t[7] + "-0"]),     # several clicks in one impression
                    " ".join([t[3] + "-1", t[4] + "-1"]),                                           # no non-clicked news
                    " ".join([t[1] + "-0", t[6] + "-1"])]                                           # a pool smaller than K
    beh = {"train": behaviours(rng, 40, 1, users, split_news["train"], hist, forced_train),
           "dev": behaviours(rng, 24, 1, users + ["U900", "U901"], split_news["dev"], hist[2:] + hist[:2]),
           "test": behaviours(rng, 24, 1, users + ["U902"], split_news["test"], hist[5:] + hist[:5])}
    for split in ("train", "dev", "test"):
        os.makedirs(os.path.join(out, split), exist_ok=True)
        with open(os.path.join(out, split, "news.tsv"), "w", encoding="utf-8") as f:
            f.writelines(lines[n] for n in split_news[split])
        with open(os.path.join(out, split, "behaviors.tsv"), "w", encoding="utf-8") as f:
            f.writelines(beh[split])
    os.makedirs(os.path.join(out, "test_unlabelled"), exist_ok=True)
    with open(os.path.join(out, "test_unlabelled", "behaviors.tsv"), "w", encoding="utf-8") as f:
        for line in beh["test"]:
            head, imps = line.rstrip("\n").rsplit("\t", 1)
            f.write(head + "\t" + " ".join(c[:-2] for c in imps.split(" ")) + "\n")
    # similarity lists: up to M = 3 other news by descending cosine, some under the 0.5 threshold; every seventh news has none
    sim = {"<PAD>": []}
    for k, nid in enumerate(ids):
        others = rng.sample([n for n in ids if n != nid], 0 if k % 7 == 3 else rng.randint(1, 3))
        cos = sorted((round(rng.uniform(0.30, 0.95), 4) for _ in others), reverse=True)
        sim[nid] = [[o, c] for o, c in zip(others, cos)]
    with open(os.path.join(out, "similarity-3.json"), "w", encoding="utf-8") as f:
        json.dump(sim, f)
    # what the fixture promises
    all_train = "".join(lines[n] for n in train_ids).lower()
    assert "quokka" not in all_train and all_train.count("zebra") == 1
    assert any(len(b.split("\t")[3]) == 0 for b in beh["train"]) and any(len(b.split("\t")[3].split(" ")) > 10 for b in beh["dev"])
    assert len({lines[n].split("\t")[1] for n in ids}) == 5
    assert any(len(v) == 0 for k, v in sim.items() if k != "<PAD>")
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(out) for f in fs)
    print("wrote %s: %d news, %d bytes" % (os.path.relpath(out, REPO), len(ids), size))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
