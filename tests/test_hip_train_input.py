"""GPU suite: the training input on the device (digat_amd/train_input.py, csrc/digat_train_input.inc) — the sampler kernel
against its numpy restatement bit for bit, a device-assembled batch against ``Trainer.gather`` on a host set holding the same
samples, and training through either input path giving the same losses."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 2, 3, 4, 5, 7, 9, 15, 16, 17, 37, 300)        # 1, 2, K-1, K, K+1 for K in {1, 4, 8, 16}, and 7, 37, 300


def pools(n, sizes, seed, news_num=5000):
    rng = np.random.default_rng(seed)
    m = np.asarray(sizes, dtype=np.int64)[rng.integers(0, len(sizes), size=n)]
    if n >= len(sizes):
        m[rng.permutation(n)[:len(sizes)]] = sizes                                # every size at least once
    off = np.r_[0, np.cumsum(m)].astype(np.int64)
    pool = rng.integers(1, news_num, size=max(int(off[-1]), 1)).astype(np.int64)
    click = rng.integers(1, news_num, size=n).astype(np.int64)
    return click, off, pool


def device_samples(click, off, pool, K, seed, epoch):
    from digat_amd import _lib
    t = [torch.from_numpy(a).to(DEV) for a in (click, off, pool)]
    out = torch.full((len(click), 1 + K), -7, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().digat_negative_sample(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(click), K, seed, epoch, out.data_ptr(),
                                                _lib.stream_ptr()), "digat_negative_sample")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("K", [1, 4, 8, 16])
def test_sampler_kernel_equals_its_host_restatement(K):
    from digat_amd.train_input import negative_samples_host
    for n in (1, 63, 64, 65, 1000):
        click, off, pool = pools(n, SIZES, seed=100 * K + n)
        got = device_samples(click, off, pool, K, seed=11, epoch=n % 3)
        assert np.array_equal(got, negative_samples_host(click, off, pool, K, seed=11, epoch=n % 3)), (K, n)


def test_sampler_kernel_with_empty_pools_and_past_the_grid_stride():
    from digat_amd.train_input import SAMPLE_GRID_THREADS, negative_samples_host
    click, off, pool = pools(300, (0, 1, 4, 5, 37), seed=5)
    got = device_samples(click, off, pool, 4, seed=2, epoch=9)
    empty = np.flatnonzero(np.diff(off) == 0)
    assert len(empty) > 0 and (got[empty] == click[empty, None]).all()
    assert np.array_equal(got, negative_samples_host(click, off, pool, 4, seed=2, epoch=9))
    # one behaviour more than the grid has threads: the first thread takes a second behaviour
    n = SAMPLE_GRID_THREADS + 1
    click, off, pool = pools(n, (1, 2, 3, 4, 5, 7, 37), seed=6)
    got = device_samples(click, off, pool, 4, seed=3, epoch=1)
    assert np.array_equal(got, negative_samples_host(click, off, pool, 4, seed=3, epoch=1))


_shared = {}


def small_corpus():
    """About 256 news and 64 impressions (the tiny task of test_hip_training.py), built once."""
    if "corpus" not in _shared:
        from digat_amd import synthetic
        spec = synthetic.SynthSpec(news_num=256, sag_neighbors=3, sag_hops=1, max_history_num=10, category_num=5, embedding_dim=64,
                                   impressions=64, mean_candidates=10.0, max_candidates=24, seed=5)
        _shared["corpus"] = synthetic.make_corpus(spec)
    return _shared["corpus"]


def paired_sets(corpus, epoch=0):
    """A device set after one sampling launch and a host set holding the same samples."""
    from digat_amd.train_input import DeviceTrainSet
    from digat_amd.trainer import SyntheticTrainSet
    dev_set = DeviceTrainSet(corpus, 4, seed=7, device=DEV)
    dev_set.negative_sampling(epoch)
    host_set = SyntheticTrainSet(corpus, 4, seed=0)
    host_set.samples[:] = dev_set.samples_host()
    return host_set, dev_set


@pytest.mark.parametrize("user_graphs", ["table", "derived"])
@pytest.mark.parametrize("titles", [False, True])
def test_device_batch_equals_the_host_gather(user_graphs, titles):
    from digat_amd import synthetic, util
    from digat_amd.train_input import epoch_order, negative_samples_host
    from digat_amd.trainer import Trainer
    corpus = small_corpus()
    dc = util.DeviceCorpus.from_numpy(corpus, torch.device(DEV), user_graphs=user_graphs)
    if titles:
        text, mask = synthetic.make_titles(corpus.spec.news_num, 16, 300, seed=7)
        dc.title_text, dc.title_mask = torch.from_numpy(text).to(torch.int32).to(DEV), torch.from_numpy(mask).to(DEV)
    host_set, dev_set = paired_sets(corpus)
    n = len(host_set)
    assert 64 < n < 128
    imp, click, off, pool = (t.cpu().numpy() for t in (dev_set.impression, dev_set.click, dev_set.pool_offsets, dev_set.pool))
    assert np.array_equal(host_set.samples, negative_samples_host(click, off, pool, 4, seed=7, epoch=0))
    order = epoch_order(n, 1)

    def trainer(train_set):
        t = object.__new__(Trainer)                      # gather needs the corpus and the set only
        t.dc, t.train_set, t.local_rank, t.batch_size = dc, train_set, -1, 64
        return t
    th, td = trainer(host_set), trainer(dev_set)
    views = list(td.batches(1))                          # uploads the order
    assert views == [(0, 64), (64, n - 64)]
    for s, B in [(0, 1), (5, 3), (0, 64), (64, n - 64)]:   # B = 1, 3, 64 and the short last batch
        want = th.gather(order[s:s + B])
        got = td.gather((s, B))
        torch.cuda.synchronize()
        assert len(got) == len(want) == 9
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and g.dtype == w.dtype and g.device == w.device, (k, s, B, g.shape, w.shape, g.dtype, w.dtype)
            assert torch.equal(g, w), (k, s, B)


def tiny_model(corpus, epochs):
    from digat_amd.model import Model, PrecomputedNewsEncoder
    spec = corpus.spec
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=2,
                                dropout_rate=0.1, epoch=epochs, batch_size=16, lr=1e-3, weight_decay=0.0, gradient_clip_norm=1.0)
    torch.manual_seed(0)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding), trainable=True))
    model.initialize()
    return model.to(DEV), cfg


def test_six_training_steps_give_the_same_losses_through_either_input_path():
    """A tiny DIGAT model, 6 steps of ``Trainer.train_step`` over the same batches: the host path fed with the device set's
    samples, twice, and the device path.  Two host runs agree bit for bit (ordered reductions, dropout seeds from torch's
    generator), and so must the device run: its inputs are the same bits."""
    from digat_amd import util
    from digat_amd.trainer import Trainer
    corpus = small_corpus()
    dc = util.DeviceCorpus.from_numpy(corpus, torch.device(DEV))

    def run(device_path):
        host_set, dev_set = paired_sets(corpus)
        model, cfg = tiny_model(corpus, 1)
        trainer = Trainer(model, cfg, dc, dev_set if device_path else host_set)
        model.train()
        torch.manual_seed(123)
        losses = []
        for k, idx in enumerate(trainer.batches(1)):
            if k == 6:
                break
            losses.append(trainer.train_step(idx))
        assert len(losses) == 6 and all(np.isfinite(losses))
        return losses
    a, b, c = run(False), run(False), run(True)
    print(f"\n[train input parity] host {a}\n                     device {c}")
    assert a == b, (a, b)
    assert c == a, (c, a)


def test_trainer_trains_two_epochs_on_the_device_input_path():
    from digat_amd import util
    from digat_amd.train_input import DeviceTrainSet, negative_samples_host
    from digat_amd.trainer import Trainer
    corpus = small_corpus()
    dc = util.DeviceCorpus.from_numpy(corpus, torch.device(DEV))
    model, cfg = tiny_model(corpus, 2)
    train_set = DeviceTrainSet(corpus, 4, seed=0, device=DEV)
    trainer = Trainer(model, cfg, dc, train_set)
    losses = trainer.train()
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert losses[1] < losses[0], losses
    # the set counted its own epochs: what it holds now is draw 1, and draw 0 was another one
    click, off, pool = (t.cpu().numpy() for t in (train_set.click, train_set.pool_offsets, train_set.pool))
    first, second = (negative_samples_host(click, off, pool, 4, seed=0, epoch=e) for e in (0, 1))
    assert train_set.epoch == 2 and np.array_equal(train_set.samples_host(), second)
    assert not np.array_equal(first, second)
