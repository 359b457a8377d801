"""Shared by tests/test_dot_topk_cpu.py and tests/test_hip_dot_topk.py: a small NRMS / NRMS-SA model with a corpus-like dev object on
``synthetic.make_nrms_inputs``, the stock score matrix and a brute-force ``sorted()`` top-k over it."""
import functools
import math
import types

import numpy as np
import torch

MODELS = {"nrms": "NRMS", "sa": "NRMS-SA"}
NEWS, AUG, LW, VOCAB, DM, HEADS, DK, ATT, USERS, HIST = 90, 2, 8, 60, 16, 4, 4, 8, 9, 6


@functools.lru_cache(maxsize=None)
def inputs(seed=3):
    from digat_amd import synthetic
    return synthetic.make_nrms_inputs(NEWS, AUG, LW, VOCAB, USERS, HIST, 5, seed=seed)


def model(pre, device="cpu", seed=11):
    from digat_amd import nrms, synthetic
    m = nrms.Model(nrms.make_config(model=MODELS[pre], dropout_rate=0.0, vocabulary_size=VOCAB, word_embedding_dim=DM, head_num=HEADS,
                                    head_dim=DK, attention_dim=ATT, max_title_length=LW, max_history_num=HIST, augmented_news_num=AUG))
    state = synthetic.make_nrms_state(VOCAB, DM, HEADS, DK, ATT, sa=(pre == "sa"), seed=seed)
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.to(device).eval()


def dev_set(device="cpu", seed=3):
    """The corpus-like object nrms.compute_scores and nrms.recommend read (no rows: recommend does not need them)."""
    t = {k: torch.from_numpy(v.astype(np.int64)).to(device) for k, v in inputs(seed).items()}
    return types.SimpleNamespace(title_text=t["title_text"], title_mask=t["title_mask"], augmented_title_text=t["augmented_title_text"],
                                 augmented_title_mask=t["augmented_title_mask"], history_ids=t["history_ids"], history_mask=t["history_mask"])


def stock_scores(m, dev, hist=None, mask=None):
    """[G, N] float32 numpy: <user, news> of every user of ``dev`` (or of the given histories) with every news, on stock PyTorch, in
    the expression of the CPU path — candidates from the augmented cache, histories from the plain one."""
    from digat_amd import nrms
    cpu = types.SimpleNamespace(**{k: v.cpu() for k, v in vars(dev).items()})
    hist = cpu.history_ids if hist is None else torch.as_tensor(hist)
    mask = cpu.history_mask if mask is None else torch.as_tensor(mask)
    with torch.no_grad():
        plain, aug = nrms.news_caches(m, cpu.title_text, cpu.title_mask, cpu.augmented_title_text, cpu.augmented_title_mask)
        user = m.user_encoder.encode_stock(plain[hist.long()], mask)
        G, N = user.shape[0], aug.shape[0]
        rows = (aug.repeat(G, 1) * user.repeat_interleave(N, dim=0)).sum(dim=1)
    return rows.view(G, N).numpy()


def brute_force(scores_g, cand, banned, k):
    """One user: the candidates ``cand`` (ids, in order) that are not banned, sorted by (NaN last, score descending, position
    ascending) as Python tuples -> [(id, score)] of the first k."""
    elems = []
    for pos, c in enumerate(int(v) for v in cand):
        if c in banned:
            continue
        x = float(scores_g[c])
        elems.append((1, 0.0, pos, c) if math.isnan(x) else (0, -x, pos, c))
    elems.sort()
    return [(e[3], np.float32(scores_g[e[3]])) for e in elems[:k]]


def banned_ids(hist_row, mask_row):
    """What exclude_history keeps from a user: its history where the mask is set, and row 0."""
    return {0} | {int(h) for h, m in zip(hist_row, mask_row) if m}


def check_rows(got_ids, got_scores, got_count, want, k):
    """``want``: per user the brute-force list; ids, score bits, counts and the -1 / -inf fill."""
    got_ids, got_scores, got_count = (np.asarray(t.cpu()) for t in (got_ids, got_scores, got_count))
    assert got_ids.shape == got_scores.shape == (len(want), k) and got_ids.dtype == np.int64 and got_scores.dtype == np.float32
    assert got_count.dtype == np.int32 and got_count.shape == (len(want),)
    for g, w in enumerate(want):
        assert got_count[g] == len(w), g
        assert got_ids[g, :len(w)].tolist() == [e[0] for e in w], g
        assert got_scores[g, :len(w)].view(np.uint32).tolist() == [int(np.float32(e[1]).view(np.uint32)) for e in w], g
        assert np.all(got_ids[g, len(w):] == -1) and np.all(np.isneginf(got_scores[g, len(w):])), g
