"""GPU suite: the encoder with its first user context on the GEMM + ``user_ctx0_kernel`` pair (csrc/digat_ctx0.inc).  On the small
synthetic corpus of test_grouped_inference_is_bit_identical_to_per_row (1024 news, 40 impressions, L = 3) the grouped entry, the
per-row entry and the shared-user entry give the same bits, and the scores agree with the fp32 CPU oracle at 2e-5 / 2e-5 as
test_hip_parity.py's corpus tests hold them (the absolute part scaled by the largest logit).  Measured on the MI355X: max |score -
oracle| 2.44e-04 at logits up to 1070 (2.3e-07 of the largest)."""
import types

import numpy as np
import pytest
import torch

from oracle import digat_oracle as O

pytestmark = pytest.mark.gpu


def test_grouped_per_row_and_shared_scores_agree_bitwise_and_with_the_oracle():
    from digat_amd import synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda:0")
    spec = synthetic.SynthSpec(news_num=1024, sag_neighbors=3, sag_hops=2, impressions=40, mean_candidates=30.0,
                               max_candidates=80, seed=77)
    corpus = synthetic.make_corpus(spec)
    L = 3
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, L, seed=78, bias_std=0.05)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num,
                                graph_depth=L, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model = model.to(dev).eval()
    enc = model.graph_encoder
    dc = util.DeviceCorpus.from_numpy(corpus, dev)
    util.prepare_news_side(enc, dc, 512)
    per_row = util.score_rows(model, dc, 0, dc.rows, 512, grouped=False)
    grouped = util.score_rows(model, dc, 0, dc.rows, 512, grouped=True)
    assert torch.equal(per_row, grouped), float((per_row - grouped).abs().max())
    # the drop-in path: the per-row entry with the encoder's own search for runs of identical users
    # (taken for batches of SHARED_USERS_MIN_ROWS rows or more whose user graphs go to the sparse Eq. 8 kernel)
    assert enc._launch_option("detect_shared_users") and enc.resolved_xattn_mode("user") == "sparse" and dc.rows >= 512 + enc.SHARED_USERS_MIN_ROWS
    with torch.no_grad():
        shared = torch.cat([model.inference(*util.gather_batch(dc, s, min(s + 512, dc.rows))) for s in range(0, dc.rows, 512)])
    assert torch.equal(shared, per_row), float((shared - per_row).abs().max())

    p = O.as_params(state)
    emb = torch.from_numpy(corpus.news_embedding)
    ids = torch.from_numpy(corpus.news_node_ID.astype(np.int64))
    sa = emb.index_select(0, ids.flatten()).view(ids.shape[0], -1, spec.embedding_dim)
    masks, graphs = torch.from_numpy(corpus.news_graph_mask), torch.from_numpy(corpus.news_graph)
    n = min(dc.rows, 192)
    with torch.no_grad():
        c_n0 = O.news_graph_context(p, sa, masks)
        imp = torch.from_numpy(corpus.row_impression[:n])
        cand = torch.from_numpy(corpus.row_candidate[:n].astype(np.int64))
        hist = torch.from_numpy(corpus.history.astype(np.int64)).index_select(0, imp)
        ue = emb.index_select(0, hist.flatten()).view(n, spec.max_history_num, spec.embedding_dim)
        want = torch.cat([O.row_logits(p, L, ue[s:s + 64], torch.from_numpy(corpus.user_graph).index_select(0, imp[s:s + 64]),
                                       torch.from_numpy(corpus.user_category_mask).index_select(0, imp[s:s + 64]),
                                       torch.from_numpy(corpus.user_category_indices).index_select(0, imp[s:s + 64]),
                                       sa.index_select(0, cand[s:s + 64]), graphs.index_select(0, cand[s:s + 64]),
                                       masks.index_select(0, cand[s:s + 64]), c_n0.index_select(0, cand[s:s + 64])) for s in range(0, n, 64)])
    g = grouped.cpu()[:n]
    print(f"encoder ctx0: max|score - oracle| {float((g - want).abs().max()):.3e}, largest |logit| {float(want.abs().max()):.3f}")
    assert torch.allclose(g, want, rtol=2e-5, atol=2e-5 * float(want.abs().max())), float((g - want).abs().max())
