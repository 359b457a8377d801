"""CPU suite: the training input path of digat_amd/train_input.py without a GPU — the two C entries are exported and refuse bad
arguments before any launch, the numpy restatement of the sampler (``negative_samples_host``, which the GPU suite holds the
kernel to bit for bit) follows the reference's rules and draws uniformly, and the device set lists the same behaviours and
visits the same batches as the host set."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

UNIFORMITY_SEED = 20261                           # picked once; the bounds below are the 5 sigma of the issue, not fitted to it


def pool_sizes(K):
    return sorted({m for m in (1, 2, K - 1, K, K + 1, 7, 37, 300) if m >= 1})


def fake_corpus(sizes, news_num=1000, seed=0):
    """One impression per pool size (cycled over 40 impressions): one clicked row and ``m`` non-clicked rows."""
    rng = np.random.default_rng(seed)
    imp, cand, lab = [], [], []
    for i in range(40):
        m = sizes[i % len(sizes)]
        imp += [i] * (m + 1)
        cand += list(1 + rng.choice(news_num - 1, size=m + 1, replace=False))      # distinct within an impression
        lab += [1] + [0] * m
    return types.SimpleNamespace(row_impression=np.array(imp, dtype=np.int64), row_candidate=np.array(cand, dtype=np.int32),
                                 row_label=np.array(lab, dtype=np.int8), news_node_ID=np.zeros((news_num, 3), dtype=np.int64),
                                 history=np.zeros((40, 5), dtype=np.int32))


def test_symbols_are_exported_and_the_twin_surface_is_untouched():
    import inspect
    from digat_amd import _ctypes_binding as T, _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    for name in ("digat_negative_sample", "digat_train_batch_ids"):
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.digat_version() == _lib.ABI_VERSION == 4
    twin = [n for n, f in vars(T).items() if inspect.isfunction(f) and f.__module__ == T.__name__ and not n.startswith("_")]
    assert len(twin) == 12 and not any("negative" in n or "train_batch" in n for n in twin)


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)
    ARG, SHAPE = 1, 2
    assert L.digat_negative_sample(None, p, p, 4, 4, 0, 0, p, None) == ARG
    assert L.digat_negative_sample(p, p, p, 4, 4, 0, 0, None, None) == ARG
    assert L.digat_negative_sample(p, p, p, 4, 0, 0, 0, p, None) == ARG
    assert L.digat_negative_sample(p, p, p, 4, 17, 0, 0, p, None) == SHAPE
    assert L.digat_negative_sample(p, p, p, -1, 4, 0, 0, p, None) == ARG
    assert L.digat_negative_sample(p, p, p, 0, 4, 0, 0, p, None) == 0          # nothing to do, no launch

    def ids(order=p, B=2, n=4, K=4, news=8, N=3, imps=8, H=5, out=p):
        return L.digat_train_batch_ids(order, B, p, p, n, K, p, news, N, p, imps, H, out, p, p, p, None)
    assert ids(order=None) == ARG and ids(out=None) == ARG
    assert ids(K=0) == ARG and ids(B=-1) == ARG and ids(n=-1) == ARG and ids(n=0) == ARG
    assert ids(K=17) == SHAPE and ids(N=0) == SHAPE and ids(H=0) == SHAPE
    assert ids(B=0) == 0


@pytest.mark.parametrize("K", [1, 4, 8])
def test_host_sampler_follows_the_reference_rules(K):
    from digat_amd.train_input import behavior_arrays, negative_samples_host
    from digat_amd.trainer import SyntheticTrainSet
    corpus = fake_corpus(pool_sizes(K), seed=K)
    imp, click, off, pool = behavior_arrays(corpus)
    m = np.diff(off)
    assert set(m) == set(pool_sizes(K))
    s = negative_samples_host(click, off, pool, K, seed=3, epoch=0)
    assert s.shape == (len(click), 1 + K) and s.dtype == np.int64
    assert np.array_equal(s[:, 0], click)
    host = SyntheticTrainSet(corpus, K, seed=0)
    host.negative_sampling()
    assert np.array_equal(host.impression, imp)
    for i in range(len(click)):
        mine = pool[off[i]:off[i + 1]]
        if m[i] <= K:
            assert np.array_equal(s[i, 1:], mine[np.arange(K) % m[i]])
            assert np.array_equal(s[i], host.samples[i])                         # the cyclic rule of the host set
        else:
            assert set(s[i, 1:]) <= set(mine) and len(set(s[i, 1:])) == K        # K distinct members of its own pool
    assert np.array_equal(s, negative_samples_host(click, off, pool, K, seed=3, epoch=0))
    assert not np.array_equal(s, negative_samples_host(click, off, pool, K, seed=3, epoch=1))
    assert not np.array_equal(s, negative_samples_host(click, off, pool, K, seed=4, epoch=0))


def test_host_sampler_handles_an_empty_pool_and_distinct_positions():
    from digat_amd.train_input import negative_samples_host
    sizes = np.array([0, 5, 0, 37, 2, 9, 300], dtype=np.int64)
    off = np.r_[0, np.cumsum(sizes)]
    pool = np.concatenate([np.arange(m) for m in sizes]).astype(np.int64)        # a member is its own position
    click = 1000 + np.arange(len(sizes), dtype=np.int64)
    for K in (1, 4, 8, 16):
        s = negative_samples_host(click, off, pool, K, seed=1, epoch=2)
        for i, m in enumerate(sizes):
            if m == 0:
                assert (s[i] == click[i]).all()
            elif m > K:
                assert len(set(s[i, 1:])) == K and s[i, 1:].max() < m and s[i, 1:].min() >= 0


@pytest.mark.parametrize("m", [5, 7, 37])
def test_host_sampler_is_uniform_over_slots_and_pairs(m):
    """200 000 behaviours with a pool of m, K = 4: every slot's position frequencies within 5 sigma of 1/m and the (slot 0,
    slot 1) pair frequencies within 5 sigma of 1/(m (m - 1)), sigma = sqrt(p (1 - p) / n)."""
    from digat_amd.train_input import negative_samples_host
    n, K = 200_000, 4
    off = np.arange(n + 1, dtype=np.int64) * m
    pool = np.tile(np.arange(m, dtype=np.int64), n)
    s = negative_samples_host(np.zeros(n, dtype=np.int64), off, pool, K, seed=UNIFORMITY_SEED, epoch=0)[:, 1:]
    assert (np.sort(s, axis=1)[:, 1:] != np.sort(s, axis=1)[:, :-1]).all()       # all picks distinct
    p = 1.0 / m
    bound = 5 * np.sqrt(p * (1 - p) / n)
    worst = 0.0
    for j in range(K):
        f = np.bincount(s[:, j], minlength=m) / n
        worst = max(worst, float(np.abs(f - p).max()) / bound)
    pp = 1.0 / (m * (m - 1))
    pbound = 5 * np.sqrt(pp * (1 - pp) / n)
    pairs = np.bincount(s[:, 0] * m + s[:, 1], minlength=m * m).reshape(m, m) / n
    assert (np.diag(pairs) == 0).all()
    pworst = float(np.abs(pairs - pp)[~np.eye(m, dtype=bool)].max()) / pbound
    print(f"\n[uniformity] pool {m}: single slot {worst:.2f}, pair {pworst:.2f} of the 5 sigma bound")
    assert worst <= 1.0, worst
    assert pworst <= 1.0, pworst


def test_device_set_lists_the_host_sets_behaviours():
    from digat_amd import synthetic
    from digat_amd.train_input import DeviceTrainSet
    from digat_amd.trainer import SyntheticTrainSet
    spec = synthetic.SynthSpec(news_num=256, sag_neighbors=3, sag_hops=1, max_history_num=10, category_num=5, embedding_dim=16,
                               impressions=64, mean_candidates=10.0, max_candidates=24, seed=5)
    corpus = synthetic.make_corpus(spec)
    host, dev = SyntheticTrainSet(corpus, 4, seed=0), DeviceTrainSet(corpus, 4, seed=0, device="cpu")
    mine = dev.behaviors
    assert len(dev) == len(host) == len(mine) > 64
    for a, b in zip(host.behaviors, mine):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert np.array_equal(dev.impression.numpy(), host.impression)
    assert dev.samples.shape == host.samples.shape and dev.samples.dtype == torch.int64
    from digat_amd import _lib
    with pytest.raises(_lib.DigatHipError):
        dev.negative_sampling()                                                  # no CPU path


@pytest.mark.parametrize("world", [1, 2, 3])
def test_shard_rule_reproduces_the_trainers_batches(world, monkeypatch):
    """``train_input.epoch_order`` against the DistributedSampler rule restated here, and ``Trainer.batches`` (either input
    path) against it, without a process group.  n = 100 with batch 16: a padded tail for world 3, a short last batch."""
    import torch.distributed as dist
    from digat_amd.train_input import epoch_order
    from digat_amd.trainer import Trainer
    n, batch, epoch = 100, 16, 3
    perm = np.random.default_rng(1000 + epoch).permutation(n)
    assert np.array_equal(epoch_order(n, epoch), perm)
    seen = []
    for rank in range(world):
        total = (n + world - 1) // world * world
        want = np.r_[perm, perm[: total - n]][rank::world]
        got = epoch_order(n, epoch, world, rank)
        assert np.array_equal(got, want) and len(got) == total // world
        seen.append(got)
        monkeypatch.setattr(dist, "get_world_size", lambda: world)
        monkeypatch.setattr(dist, "get_rank", lambda r=rank: r)
        for on_device in (False, True):
            t = object.__new__(Trainer)
            t.local_rank, t.batch_size = rank, batch
            t.train_set = type("Set", (), {"on_device": on_device, "__len__": lambda self: n})()
            t.dc = types.SimpleNamespace(news_embedding=torch.zeros(1))
            got_batches = list(t.batches(epoch))
            want_batches = [want[s:s + batch] for s in range(0, len(want), batch)]
            assert len(got_batches) == len(want_batches)
            for g, w in zip(got_batches, want_batches):
                if on_device:
                    assert np.array_equal(t.order_dev.numpy()[g[0]:g[0] + g[1]], w)
                else:
                    assert np.array_equal(g, w)
    assert set(np.concatenate(seen)) == set(range(n))
