#!/usr/bin/env python3
"""Mint ``tests/golden/sag_tiny_golden.npz``: what the REAL reference's ``construct_SAG.py`` makes of ``tests/golden/sag_tiny``.

Runs only where the reference tree is readable, and writes data only.  For ``dataset_type`` ``'small'`` and ``'large'`` it plants
the fixture's embeddings as the reference's pickle caches in a temporary directory and runs the reference's own driver there:
``generate_semantic_embeddings`` (the news bookkeeping; the sentence model is a ``sentence_transformers`` stub that is never
called), ``generate_similariy_info``, ``generate_similar_news_list``, ``aggregate`` and ``generate_news_graph``.  One step is
replaced: ``generate_cos_similarities`` moves its tensors to ``.cuda()``, so ``oracle.sag_oracle.generate_cos_similarities`` stands
in for it (the ``sag_cos_*`` goldens hold that function to the reference's).  The golden's ``meta`` says so.

Stored per dataset type ``<t>`` and category ``<c>``: ``<t>/<c>/meta_<mode>`` (json of the five news_meta items), ``<t>/<c>/avg_values``
/ ``avg_indices`` (the average top-k); per dataset type the aggregated lists as arrays (``sim_index`` / ``sim_cos`` / ``sim_len``),
``empty_rows`` (the news with no text, whose neighbours the reference draws at random) and ``news_node_ID`` / ``news_graph`` /
``news_graph_mask``.

The tool ASSERTS the fixture's separation, so that a comparison of indices needs no exclusions: in every average top-k row
neighbouring values differ by more than 2e-5, the first value left out (rank k + 1) included, and no value lies within 1e-4 of the
0.5 threshold.  If an assert fails, pick another seed in ``tools/make_sag_fixture.py``.

Usage:  python tools/mint_sag_golden.py
"""
from __future__ import annotations

import json
import os
import pickle
import shutil
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
FIXTURE = os.path.join(REPO, "tests", "golden", "sag_tiny")
OUT = os.path.join(REPO, "tests", "golden", "sag_tiny_golden.npz")
TOP_M, HOPS = 5, 2
GAP, THRESHOLD_MARGIN = 2e-5, 1e-4

from digat_amd import construct_SAG as ours, mind, synthetic  # noqa: E402
import sag_oracle  # noqa: E402


def main():
    import make_golden
    make_golden.import_reference()
    import construct_SAG as ref
    roots = [os.path.join(FIXTURE, s) for s in mind.SPLITS]
    dictionaries = mind.build_dictionaries(mind.read_news(roots), roots[0], 1)
    news_ID, category = dictionaries["news_ID"], dictionaries["category"]
    node_num = synthetic.news_graph_size(TOP_M, HOPS)
    out = {"meta": np.array(json.dumps({
        "top_M": TOP_M, "hops": HOPS, "news_node_num": node_num,
        "cos_step": "oracle.sag_oracle.generate_cos_similarities in place of the reference's generate_cos_similarities (.cuda())",
        "separation": {"gap": GAP, "threshold_margin": THRESHOLD_MARGIN}})),
        "news_ID": np.array(json.dumps(news_ID)), "category": np.array(json.dumps(category))}
    cwd = os.getcwd()
    for dataset in ("small", "large"):
        work = tempfile.mkdtemp(prefix="mint_sag_")
        recorded = {}

        def cos_step(dataset_type, top_M, cat, title, content, corpus_title, corpus_content):
            got = sag_oracle.generate_cos_similarities(title, content, corpus_title, corpus_content, top_M)
            values, indices = got["average"]
            k, m = values.shape[1], corpus_title.size(0)
            wider = sag_oracle.generate_cos_similarities(title, content, corpus_title, corpus_content, k)["average"][0].numpy()
            assert wider.shape[1] == min(k + 1, m) and np.array_equal(wider[:, :k], values.numpy())
            gaps = -np.diff(wider.astype(np.float64), axis=1)
            assert gaps.size == 0 or gaps.min() > GAP, f"{dataset_type}/{cat}: neighbouring values {gaps.min():.3e} apart; change the fixture's seed"
            margin = np.abs(values.numpy().astype(np.float64) - ref.similarity_threshold).min()
            assert margin > THRESHOLD_MARGIN, f"{dataset_type}/{cat}: a value {margin:.3e} from the threshold; change the fixture's seed"
            print(f"  {dataset_type}/{cat}: n {values.shape[0]} m {m} k {k}  min gap {gaps.min() if gaps.size else float('nan'):.3e}  "
                  f"threshold margin {margin:.3e}")
            recorded[cat] = (values.numpy(), indices.numpy())
            return tuple(t for kind in sag_oracle.KINDS for t in got[kind])

        try:
            os.chdir(work)
            for sub in ours.EMBEDDING_DIRS.values():
                os.makedirs(os.path.join(dataset + "-SAG", sub))
                src = os.path.join(FIXTURE, dataset + "-SAG", sub)
                for name in os.listdir(src):
                    with open(os.path.join(dataset + "-SAG", sub, name[:-4] + ".pkl"), "wb") as f:
                        pickle.dump(torch.from_numpy(np.load(os.path.join(src, name))), f, protocol=4)
            with open("category-%s.json" % dataset, "w", encoding="utf-8") as f:
                json.dump(category, f)
            with open("news_ID-%s.json" % dataset, "w", encoding="utf-8") as f:
                json.dump(news_ID, f)
            ref.generate_cos_similarities = cos_step
            np.random.seed(0)                                                    # the reference's draw for the news with no text
            node_ID, graph, mask = ref.construct_SAG(dataset, roots[0], roots[1], roots[2], TOP_M, HOPS, node_num, news_ID)
            with open("%s-SAG/similarity-%d.json" % (dataset, TOP_M), encoding="utf-8") as f:
                similarity = json.load(f)
            assert set(similarity) == set(news_ID)
            empty = []
            for cat in category:
                for mode, sub in ours.EMBEDDING_DIRS.items():
                    path = "%s-SAG/%s/news_meta-%s.json" % (dataset, sub, cat)
                    if os.path.exists(path):
                        with open(path, encoding="utf-8") as f:
                            meta = json.load(f)
                        out["%s/%s/meta_%s" % (dataset, cat, mode)] = np.array(json.dumps(meta))
                        if mode == "full":
                            empty += [news_ID[x] for x in meta["empty_news_IDs"]]
                if cat in recorded:
                    out["%s/%s/avg_values" % (dataset, cat)], out["%s/%s/avg_indices" % (dataset, cat)] = recorded[cat]
            sim_index, sim_cos, sim_len = sag_oracle.lists_from_dict(similarity, news_ID, TOP_M)
            out.update({dataset + "/sim_index": sim_index, dataset + "/sim_cos": sim_cos, dataset + "/sim_len": sim_len,
                        dataset + "/empty_rows": np.array(sorted(empty), dtype=np.int32), dataset + "/news_node_ID": node_ID,
                        dataset + "/news_graph": graph, dataset + "/news_graph_mask": mask})
            print("%s: %d news, lists of %s entries, graphs of up to %d nodes" % (dataset, len(news_ID), np.bincount(sim_len).tolist(),
                                                                              int(mask.sum(axis=1).max())))
        finally:
            os.chdir(cwd)
            shutil.rmtree(work, ignore_errors=True)
    np.savez_compressed(OUT, **out)
    print("wrote %s  %.1f KiB" % (os.path.relpath(OUT, REPO), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
