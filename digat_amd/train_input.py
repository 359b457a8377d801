"""Training input on the device: an epoch's negative samples and a step's tensors without host work per step.

``DeviceTrainSet`` is the device-resident twin of ``trainer.SyntheticTrainSet``: the same behaviours in the same order, with
the clicked news, the impression and the non-clicked pools (CSR) held on the device.  ``negative_sampling`` is one launch of
``digat_negative_sample`` (csrc/digat_train_input.inc) per epoch, where the host set walks the behaviours in a Python loop;
``Trainer.gather`` then assembles a step from ``(offset, length)`` views into the epoch's uploaded order with two launches
(``digat_train_batch_ids``, ``digat_gather_tables``) — no numpy, no pinned staging buffer, no host-to-device copy per step.

The sampler draws from a counter hash, not from numpy's generator: for pools larger than K the two sets draw different (equally
distributed) samples.  ``negative_samples_host`` restates the kernel in numpy, bit for bit; the tests hold the kernel to it and
it to the distribution (distinct picks, uniform slots and pairs).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

MAX_NEGATIVES = 16                      # csrc/digat_train_input.inc: NEG_MAX_K
SAMPLE_GRID_THREADS = 1024 * 256        # ... NEG_MAX_BLOCKS workgroups of 256 threads: more behaviours than this take the grid stride
_M32 = np.uint64(0xFFFFFFFF)


def _hash32(x: np.ndarray) -> np.ndarray:
    """csrc/digat_kernels.hip: hash32, on uint64 arrays holding 32-bit values."""
    x = x & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def epoch_seed(seed: int, epoch: int) -> int:
    """The epoch folded into the seed: hash32(seed ^ hash32(epoch + 0x9E3779B9))."""
    e = _hash32(np.array([(int(epoch) + 0x9E3779B9) & 0xFFFFFFFF], dtype=np.uint64))
    return int(_hash32(np.array([int(seed) & 0xFFFFFFFF], dtype=np.uint64) ^ e)[0])


def draw_words(seed: int, epoch: int, counters: np.ndarray) -> np.ndarray:
    """The 32-bit word of every counter e = i K + j (uint64 array out): drop_keep's construction,
    hash32((uint32)e * 0x9E3779B9 + hash32(seed' + (uint32)(e >> 32)))."""
    e = np.asarray(counters, dtype=np.uint64)
    inner = _hash32(np.uint64(epoch_seed(seed, epoch)) + (e >> np.uint64(32)))
    return _hash32(((e & _M32) * np.uint64(0x9E3779B9) & _M32) + inner)


def negative_samples_host(click, pool_offsets, pool, K: int, seed: int, epoch: int) -> np.ndarray:
    """``digat_negative_sample`` in numpy, bit for bit: ``samples`` [n, 1+K] int64.

    Column 0 is the click.  A pool of 1 <= m <= K members is cycled (``pool_i[j % m]``); an empty pool gives the click in every
    column.  For m > K, draw j of behaviour i takes the word w of counter i K + j, r = j + (w (m - j) >> 32), and picks the
    value at position r of a Fisher-Yates shuffle of 0 .. m-1 that exists only as the moves made so far: the value at a position
    is that of the last move onto it, else the position itself; after the pick the value at position j moves to r."""
    click = np.asarray(click, dtype=np.int64)
    off = np.asarray(pool_offsets, dtype=np.int64)
    pool = np.asarray(pool, dtype=np.int64)
    n, K = int(click.shape[0]), int(K)
    if K < 1 or K > MAX_NEGATIVES:
        raise ValueError(f"K must be in [1, {MAX_NEGATIVES}]")
    out = np.empty((n, 1 + K), dtype=np.int64)
    out[:, 0] = click
    m = off[1:] - off[:-1]
    lo = off[:-1]
    empty, cyc, big = np.flatnonzero(m <= 0), np.flatnonzero((m >= 1) & (m <= K)), np.flatnonzero(m > K)
    out[empty, 1:] = click[empty, None]
    if len(cyc):
        out[cyc, 1:] = pool[lo[cyc, None] + np.arange(K)[None, :] % m[cyc, None]]
    if len(big):
        mb = np.minimum(m[big], 0x7FFFFFFF).astype(np.uint64)
        i = big.astype(np.uint64)
        pos, val = [], []
        for j in range(K):
            w = draw_words(seed, epoch, i * np.uint64(K) + np.uint64(j))
            r = np.uint64(j) + ((w * (mb - np.uint64(j))) >> np.uint64(32))
            vr, vj = r.copy(), np.full_like(r, j)
            for p, v in zip(pos, val):                     # in move order: a later move onto the same position wins
                vr = np.where(p == r, v, vr)
                vj = np.where(p == np.uint64(j), v, vj)
            pos.append(r)
            val.append(vj)
            out[big, 1 + j] = pool[lo[big] + vr.astype(np.int64)]
    return out


def behavior_arrays(corpus) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The training behaviours of a corpus as arrays (both train sets are built from them): one behaviour per clicked row of an
    impression that has at least one non-clicked row, in row order.  -> ``(impression [n], click [n], pool_offsets [n+1])``
    int64 and ``pool`` in the candidates' dtype, the pool of a behaviour being its impression's non-clicked candidates in row
    order."""
    imp, cand, lab = np.asarray(corpus.row_impression), np.asarray(corpus.row_candidate), np.asarray(corpus.row_label)
    bounds = np.r_[0, np.flatnonzero(np.diff(imp)) + 1, len(imp)] if len(imp) else np.zeros(1, dtype=np.int64)
    imps, clicks, sizes, pools = [], [], [], []
    for s, e in zip(bounds[:-1], bounds[1:]):
        pos, negs = cand[s:e][lab[s:e] == 1], cand[s:e][lab[s:e] == 0]
        if len(negs) == 0:
            continue
        for c in pos:
            imps.append(int(imp[s]))
            clicks.append(int(c))
            sizes.append(len(negs))
            pools.append(negs)
    offsets = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(np.asarray(sizes, dtype=np.int64), out=offsets[1:])
    pool = np.concatenate(pools) if pools else np.zeros(0, dtype=cand.dtype)
    return np.asarray(imps, dtype=np.int64), np.asarray(clicks, dtype=np.int64), offsets, pool


def epoch_order(n: int, epoch: int, world_size: int = 1, rank: int = 0) -> np.ndarray:
    """The behaviours one rank visits in ``epoch``, in order: the epoch's permutation of all n, and under data parallelism its
    strided shard after padding with the permutation's head to a multiple of the world size (DistributedSampler's rule).
    ``Trainer.batches`` cuts this into batches for either input path."""
    order = np.random.default_rng(1000 + epoch).permutation(n)
    if world_size > 1 or rank > 0:
        total = (n + world_size - 1) // world_size * world_size
        order = np.r_[order, order[: total - n]][rank::world_size]
    return order


class DeviceTrainSet:
    """``SyntheticTrainSet`` with its arrays on ``device``: ``click`` / ``impression`` [n], the CSR pool and ``samples``
    [n, 1+K], all int64.  ``negative_sampling`` is one kernel launch on the current stream (nothing is read back); a set built
    with ``device="cpu"`` holds the same arrays for inspection and cannot sample (there is no CPU path)."""
    on_device = True

    def __init__(self, corpus, negative_sample_num: int = 4, seed: int = 0, device="cuda"):
        if not 1 <= int(negative_sample_num) <= MAX_NEGATIVES:
            raise ValueError(f"negative_sample_num must be in [1, {MAX_NEGATIVES}]")
        self.neg, self.seed, self.epoch = int(negative_sample_num), int(seed) & 0xFFFFFFFF, 0
        imp, click, offsets, pool = behavior_arrays(corpus)
        # checked once here, so that no launch has to: every id the step's kernels index a corpus table with
        news_num, impressions = int(corpus.news_node_ID.shape[0]), int(corpus.history.shape[0])
        for name, a, count in (("clicked news", click, news_num), ("pool news", pool, news_num), ("impression", imp, impressions)):
            if len(a) and (a.min() < 0 or a.max() >= count):
                raise ValueError(f"{name} id outside [0, {count})")
        self.device = torch.device(device)
        up = lambda a: torch.from_numpy(a.astype(np.int64)).to(self.device)
        self.impression, self.click, self.pool_offsets = up(imp), up(click), up(offsets)
        self.pool = up(pool if len(pool) else np.zeros(1))                       # never an empty allocation: the entry takes no null
        self.samples = torch.zeros((len(click), 1 + self.neg), dtype=torch.int64, device=self.device)

    @property
    def behaviors(self):
        """``SyntheticTrainSet.behaviors``: (impression, clicked, [non-clicked]) per behaviour (read back from the device)."""
        imp, click, off = self.impression.cpu().numpy(), self.click.cpu().numpy(), self.pool_offsets.cpu().numpy()
        pool = self.pool.cpu().numpy()
        return [(int(imp[i]), int(click[i]), pool[off[i]:off[i + 1]]) for i in range(len(click))]

    def negative_sampling(self, epoch: Optional[int] = None):
        """This epoch's samples: one launch.  Without an argument the set counts its own calls (0, 1, ...), which is what
        ``Trainer.train`` relies on; ``epoch`` names the draw explicitly and moves the counter behind it."""
        from . import _lib
        _lib.require_device(self.samples)
        e = self.epoch if epoch is None else int(epoch)
        if len(self):
            _lib.check(_lib.lib().digat_negative_sample(self.click.data_ptr(), self.pool_offsets.data_ptr(), self.pool.data_ptr(), len(self),
                                                        self.neg, self.seed, e & 0xFFFFFFFF, self.samples.data_ptr(), _lib.stream_ptr()),
                       "digat_negative_sample")
        self.epoch = e + 1

    def samples_host(self) -> np.ndarray:
        return self.samples.cpu().numpy()

    def __len__(self):
        return int(self.click.shape[0])


_ones = {}


def ones_mask(shape, device) -> torch.Tensor:
    """The all-true mask of a synthetic step (titles are news ids: nothing is padded), one tensor per shape and device.  Shared
    between steps: read-only by contract, as every input of ``Model.forward`` is."""
    key = (tuple(shape), str(device))
    t = _ones.get(key)
    if t is None:
        t = _ones[key] = torch.ones(tuple(shape), dtype=torch.bool, device=device)
    return t


def device_batch(dc, train_set: DeviceTrainSet, order: torch.Tensor, offset: int, length: int):
    """The 9 inputs of ``Model.forward`` for the behaviours ``order[offset : offset + length]`` — ``Trainer.gather``'s tuple,
    same shapes, dtypes and values — from two launches on the current stream: ``digat_train_batch_ids`` writes the step's index
    lists, one ``digat_gather_tables`` call gathers every large row through them (a corpus without user-graph tables adds
    ``digat_user_graph_build``).  Outputs come from torch's caching allocator, fresh every step (autograd may keep a step's
    inputs past the next step's gather, so no ring of reused buffers); nothing is copied from or read back to the host."""
    from . import _lib, util
    dev = _lib.require_device(order, train_set.samples, dc.news_node_ID, dc.history)
    n, B, K1 = len(train_set), int(length), 1 + train_set.neg
    if order.dtype != torch.int64 or not order.is_contiguous() or offset < 0 or B < 0 or offset + B > order.numel():
        raise _lib.DigatHipError("order must be a contiguous int64 tensor that holds [offset, offset + length)")
    N, H = int(dc.news_node_ID.shape[1]), int(dc.history.shape[1])
    ids = torch.empty(B * (1 + K1 + K1 * N + H), dtype=torch.int64, device=dev)          # imp | news | node_ids | hist
    imp, news, node_ids, hist = torch.split(ids, [B, B * K1, B * K1 * N, B * H])
    L = _lib.lib()
    if B:
        for t in (dc.news_node_ID, dc.history, dc.user_category_indices):
            if t.dtype != torch.int64 or not t.is_contiguous():
                raise _lib.DigatHipError("the corpus's index tables must be contiguous int64")
        _lib.check(L.digat_train_batch_ids(order.data_ptr() + 8 * offset, B, train_set.impression.data_ptr(), train_set.samples.data_ptr(), n,
                                           train_set.neg, dc.news_node_ID.data_ptr(), int(dc.news_node_ID.shape[0]), N, dc.history.data_ptr(),
                                           int(dc.history.shape[0]), H, imp.data_ptr(), news.data_ptr(), node_ids.data_ptr(), hist.data_ptr(),
                                           _lib.stream_ptr()), "digat_train_batch_ids")
    jobs = []

    def gathered(table, idx, lead):
        """rows ``idx`` of ``table`` as a new [*lead, *table.shape[1:]] tensor (one job of the step's gather)."""
        out = torch.empty((*lead, *table.shape[1:]), dtype=table.dtype, device=dev)
        if not table.is_contiguous():
            raise _lib.DigatHipError("corpus tables must be contiguous")
        jobs.append((table.data_ptr(), out.data_ptr(), table[0].numel() * table.element_size(), idx.numel(), idx.data_ptr(), 0, 1))
        return out
    table_graphs = dc.user_graph is not None
    if table_graphs:
        user_graph, cat_mask = gathered(dc.user_graph, imp, (B,)), gathered(dc.user_category_mask, imp, (B,))
    cat_idx = gathered(dc.user_category_indices, imp, (B,))
    news_graph, news_mask = gathered(dc.news_graph, news, (B, K1)), gathered(dc.news_graph_mask, news, (B, K1))
    if dc.title_text is not None:
        ht, hm = gathered(dc.title_text, hist, (B, H)), gathered(dc.title_mask, hist, (B, H))
        nt, nm = gathered(dc.title_text, node_ids, (B, K1, N)), gathered(dc.title_mask, node_ids, (B, K1, N))
    else:
        ht, nt = hist.view(B, H, 1), node_ids.view(B, K1, N, 1)
        hm, nm = ones_mask(ht.shape, dev), ones_mask(nt.shape, dev)
    if B:
        arr = (_lib.GatherJob * len(jobs))(*[_lib.GatherJob(*j) for j in jobs])
        _lib.check(L.digat_gather_tables(arr, len(jobs), _lib.stream_ptr()), "digat_gather_tables")
    if not table_graphs:
        user_graph, cat_mask = util.user_side_rows(dc, imp)
    return ht, hm, user_graph, cat_mask, cat_idx, nt, nm, news_graph, news_mask
