#!/usr/bin/env python3
"""Mint ``tests/golden/mind_tiny_golden.npz``: what the REAL reference makes of ``tests/golden/mind_tiny``.

Runs only where the reference tree is readable.  In a temporary directory it runs the reference's ``MIND_Corpus.preprocess`` and
``MIND_Corpus(config)`` on the fixture and stores their dictionaries and arrays; then a seeded state dict, the scores / ranks /
metrics of the reference's MSA + DIGAT model on the dev split (the flow of ``oracle/make_golden.py``'s ``reference_scores`` behind
the reference's news encoder) and the reference's first training-step loss with dropout 0.  Only data is written.

Stand-ins (``sys.modules`` stubs, as ``oracle/make_golden.py`` sets them up):
  * ``torchtext.vocab.GloVe``: a small seeded table covering most of the fixture's words (the rest take the reference's
    ``torch.normal`` branch, :106);
  * ``sentence_transformers``: imported by ``construct_SAG.py``, never called — the SAG's embedding steps are replaced by the
    fixture's ``similarity-3.json``, and only ``construct_SAG.generate_news_graph`` runs, on that file.
Training behaviours whose impression has no non-clicked news are taken out before the reference's sampler runs (it divides by
zero on them, MIND_dataset.py:36); their indices are stored as ``train_skipped``.

Usage:  python tools/mint_mind_golden.py
"""
from __future__ import annotations

import io
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
FIXTURE = os.path.join(REPO, "tests", "golden", "mind_tiny")
OUT = os.path.join(REPO, "tests", "golden", "mind_tiny_golden.npz")

from digat_amd import mind, synthetic  # noqa: E402

# devset_tiny's shapes; d = 64 as 4 heads x 16
CFG = dict(dataset="MIND-small", word_threshold=3, max_title_length=8, word_embedding_dim=20, SAG_hops=1, SAG_neighbors=3,
           news_graph_size=4, max_history_num=10, negative_sample_num=4, news_encoder="MSA", graph_encoder="DIGAT", MSA_head_num=4,
           MSA_head_dim=16, attention_dim=32, graph_depth=2, dropout_rate=0.0, batch_size=16)
STATE_SEED, TRAIN_BATCH = 71, 16


class TinyGloVe:
    """``GloVe(name=, dim=, cache=, max_vectors=)`` with ``stoi`` / ``vectors``: every fourth fixture word is left out."""

    def __init__(self, name=None, dim=20, cache=None, max_vectors=None):
        words = set()
        for split in mind.SPLITS:
            with open(os.path.join(FIXTURE, split, "news.tsv"), encoding="utf-8") as f:
                for line in f:
                    words.update(mind.tokenize(line.split("\t")[3]))
        words = [w for k, w in enumerate(sorted(words)) if k % 4 != 3]
        self.stoi = {w: k for k, w in enumerate(words)}
        self.vectors = torch.from_numpy(np.random.default_rng(5).standard_normal((len(words), dim)).astype(np.float32) * 0.4)


def main():
    import make_golden
    ge, ev = make_golden.import_reference()
    import MIND_corpus
    import MIND_dataset
    import construct_SAG
    import model as ref_model
    MIND_corpus.GloVe = TinyGloVe
    work = tempfile.mkdtemp(prefix="mint_mind_")
    cwd = os.getcwd()
    try:
        for split in mind.SPLITS:
            shutil.copytree(os.path.join(FIXTURE, split), os.path.join(work, "MIND-small", split))
        os.makedirs(os.path.join(work, "run"))
        os.chdir(os.path.join(work, "run"))
        cfg = types.SimpleNamespace(**CFG, train_root="../MIND-small/train", dev_root="../MIND-small/dev", test_root="../MIND-small/test")

        def sag_from_file(dataset, train_root, dev_root, test_root, top_M, hop, node_num, news_ID_dict):
            with open(os.path.join(FIXTURE, "similarity-3.json"), encoding="utf-8") as f:
                return construct_SAG.generate_news_graph(dataset, json.load(f), news_ID_dict, top_M, hop, node_num)
        MIND_corpus.construct_SAG = sag_from_file
        torch.manual_seed(3)
        MIND_corpus.MIND_Corpus.preprocess(cfg)
        corpus = MIND_corpus.MIND_Corpus(cfg)
        out = {}
        for name in ("user_ID", "news_ID", "category", "subCategory", "word"):
            out["dict_" + name] = np.array(json.dumps(getattr(corpus, name + "_dict")))
        # the category of every news as preprocess step 6 reads it (:131-135)
        news_category = np.zeros(corpus.news_num, dtype=np.int64)
        for root in (cfg.train_root, cfg.dev_root, cfg.test_root):
            with open(os.path.join(root, "news.tsv"), encoding="utf-8") as f:
                for line in f:
                    nid, cat = line.split("\t")[:2]
                    news_category[corpus.news_ID_dict[nid]] = corpus.category_dict[cat]
        with open("word_embedding-3-20-8-MIND-small.pkl", "rb") as f:
            import pickle
            out["word_embedding"] = pickle.load(f).numpy()
        out.update(news_title_text=corpus.news_title_text, news_title_mask=corpus.news_title_mask, news_category=news_category,
                   news_node_ID=corpus.news_node_ID, news_graph=corpus.news_graph, news_graph_mask=corpus.news_graph_mask)
        for split in mind.SPLITS:
            for part in ("graph", "graph_mask", "category_mask", "category_indices"):
                out[f"{split}_user_history_{part}"] = getattr(corpus, f"{split}_user_history_{part}")
        for split in ("dev", "test"):
            beh = getattr(corpus, split + "_behaviors")
            out[split + "_history"] = np.array([b[0] for b in beh], dtype=np.int32)
            out[split + "_candidate"] = np.array([b[1] for b in beh], dtype=np.int64)
            out[split + "_indices"] = np.array(getattr(corpus, split + "_indices"), dtype=np.int64)
        tb = corpus.train_behaviors
        out.update(train_history=np.array([b[0] for b in tb], dtype=np.int32), train_click=np.array([b[1] for b in tb], dtype=np.int64),
                   train_behavior_index=np.array([b[3] for b in tb], dtype=np.int64),
                   train_pool=np.array([n for b in tb for n in b[2]], dtype=np.int64),
                   train_pool_offsets=np.cumsum([0] + [len(b[2]) for b in tb]).astype(np.int64),
                   train_skipped=np.array([k for k, b in enumerate(tb) if not b[2]], dtype=np.int64))

        # ---- the reference's MSA + DIGAT model with a seeded state
        cfg.vocabulary_size, cfg.category_num = len(corpus.word_dict), len(corpus.category_dict)
        d = cfg.MSA_head_num * cfg.MSA_head_dim
        state = {"news_encoder." + k: v for k, v in synthetic.make_msa_state(cfg.vocabulary_size, cfg.word_embedding_dim, cfg.MSA_head_num,
                                                                            cfg.MSA_head_dim, cfg.attention_dim, seed=STATE_SEED).items()}
        state.update({"graph_encoder." + k: v for k, v in synthetic.make_state_dict(d, cfg.category_num, cfg.graph_depth, seed=STATE_SEED + 1,
                                                                                   bias_std=0.05).items()})
        model = ref_model.Model(cfg)
        model.initialize()
        res = model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        out.update({"w_" + k: v for k, v in state.items()})
        model.eval()
        with torch.no_grad():                                                       # util.py:24-33
            emb = model.news_encoder(torch.from_numpy(corpus.news_title_text).long().unsqueeze(1),
                                     torch.from_numpy(corpus.news_title_mask).unsqueeze(1)).squeeze(1).numpy()
        dev = types.SimpleNamespace(news_embedding=emb, news_node_ID=corpus.news_node_ID, news_graph=corpus.news_graph,
                                    news_graph_mask=corpus.news_graph_mask, history=out["dev_history"][np.r_[True, np.diff(out["dev_indices"]) != 0]],
                                    user_graph=corpus.dev_user_history_graph, user_category_mask=corpus.dev_user_history_category_mask,
                                    user_category_indices=corpus.dev_user_history_category_indices, row_impression=out["dev_indices"],
                                    row_candidate=out["dev_candidate"], rows=len(out["dev_indices"]))
        scores, _ = make_golden.reference_scores(model.graph_encoder, dev, 64)
        with open(os.path.join(FIXTURE, "dev", "behaviors.tsv"), encoding="utf-8") as f:
            labels = [[int(t[-1]) for t in line.split("\t")[4].strip().split(" ")] for line in f]
        sub = [[] for _ in labels]                                                 # util.py:70-80
        for i, imp in enumerate(out["dev_indices"].tolist()):
            sub[imp].append([float(scores[i]), len(sub[imp])])
        lines, truth = [], []
        for i, s in enumerate(sub):
            s.sort(key=lambda x: x[0], reverse=True)
            rank = [0] * len(s)
            for j in range(len(s)):
                rank[s[j][1]] = j + 1
            lines.append(str(i + 1) + " " + str(rank).replace(" ", ""))
            truth.append(str(i + 1) + " " + str(labels[i]).replace(" ", ""))
        metrics = ev.scoring(io.StringIO("\n".join(truth)), io.StringIO("\n".join(lines)))
        print("dev: rows=%d AUC=%.6f MRR=%.6f nDCG5=%.6f nDCG10=%.6f" % ((len(scores),) + tuple(metrics)))
        out.update(dev_news_embedding=emb.astype(np.float32), dev_scores=scores.astype(np.float32), dev_rank_lines=np.array("\n".join(lines)),
                   dev_label=np.array([v for row in labels for v in row], dtype=np.int8), dev_metrics=np.array(metrics, dtype=np.float64))

        # ---- the first training step (trainer.py:88-100), dropout 0: the first TRAIN_BATCH behaviours that have a pool, in order
        corpus.train_behaviors = [b for b in tb if b[2]]
        train = MIND_dataset.MIND_Train_Dataset(corpus)
        np.random.seed(11)
        train.negative_sampling(verbose=False)
        samples = np.array(train.train_samples, dtype=np.int64)
        items = [train[i] for i in range(TRAIN_BATCH)]
        batch = [torch.from_numpy(np.stack([np.asarray(it[k]) for it in items])) for k in range(10)]
        (ut, um, ug, _ugm, ucm, uci, nt, nm, ng, ngm) = batch
        model.train()
        logits = model(ut.long(), um, ug, ucm, uci, nt.long(), nm, ng, ngm)
        loss = (-torch.log_softmax(logits, dim=1).select(1, 0)).mean()
        print("first training step: loss %.8f" % float(loss.detach()))
        out.update(train_samples=samples, train_batch=np.arange(TRAIN_BATCH, dtype=np.int64), train_logits=logits.detach().numpy(),
                   train_loss=np.float64(float(loss.detach())))
        out["config"] = np.array(json.dumps(CFG))
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
    np.savez_compressed(OUT, **out)
    print("wrote %s  %.1f KiB" % (os.path.relpath(OUT, REPO), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
