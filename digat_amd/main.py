"""Entry point: ``python -m digat_amd.main --mode={train,dev,test} --graph_encoder=DIGAT ...``

The counterpart of the reference's ``main.py``, on a synthetic MIND-shaped corpus or — ``--data_root`` — on MIND files read by
``mind.load`` (the model then has its text encoder, ``--news_encoder MSA|CNN``; trained on the train split, selected on dev, saved
under ``--model_dir``; ``test`` / ``recommend`` run on the test split, an unlabelled one gives the rank file and no metrics): ``train`` runs the
``Trainer`` (DDP when launched with one process per GPU) and then scores the dev rows; ``dev`` / ``test`` load
``--dev_model_path`` / ``--test_model_path`` (the ``{model_name: state_dict}`` file the ``Trainer`` writes, main.py:23,36),
score the rows and print AUC / MRR / nDCG@5 / nDCG@10 and the inference time (main.py:66-72); ``test`` writes the rank file
to ``--test_output_file`` when one is named.  ``recommend`` loads ``--test_model_path`` as ``test`` does and, for every impression of the
corpus, picks the ``--recommend_k`` best of ALL non-PAD news the impression's user has not read (``util.recommend``); it writes
``"<impression id> [id1,id2,...]"`` per line — the rank file's framing — to ``--recommend_output`` when one is named.
``--recommend_diversity F`` makes those the k maximal-marginal-relevance picks of a shortlist (``--recommend_shortlist``), with
``--recommend_max_per_category Q`` at most Q of one category — on a corpus that carries the news' categories (MIND does).
``--recommend_calibration F`` instead makes them the k picks of a shortlist of up to 1024 (``--recommend_shortlist``) that keep the
category mix of the reader's history (``util.recommend(calibration=)``) — on a corpus that carries the news' categories.
``--recommend_sample T`` instead DRAWS them: one Plackett-Luce slate per impression from ``softmax(score / T)`` over that shortlist
(``util.recommend(sample=)``, ``--recommend_seed``).
``--recommend_rerank D,C`` instead makes them diverse AND calibrated in one greedy pass over that shortlist (``util.recommend(rerank=)``;
``--recommend_max_per_category`` composes).
``--recommend_exposure_cap N`` instead bounds how often a news is shown: no news in more than N of the lists written, every list the
best k of that shortlist among the news that still have room for it (``util.recommend(exposure_cap=)``; the cap holds over the run).
``--recommend_report 0,0.1,0.3`` then prints one line per diversity with what the knob buys and costs (``util.recommend_report``: one
scoring pass for all of them; on a labelled split the accuracy of the lists against each impression's clicked candidates as well).
``--bootstrap B`` (``dev`` / ``test`` on a labelled split) prints, below the four metrics, one line per metric with its percentile
interval from B bootstrap replicates over impressions (``--bootstrap_level``, ``--seed``); ``--compare_model_path PATH`` loads a
second checkpoint of the same architecture and prints the paired bootstrap of the differences (``evaluate.compare_metrics``).
"""
from __future__ import annotations

import time

import numpy as np
import torch

from . import synthetic, util
from .config import Config
from .model import Model, PrecomputedNewsEncoder
from .trainer import SyntheticTrainSet, Trainer


def load_checkpoint(model, path: str) -> None:
    """Load the ``{model_name: state_dict}`` file ``Trainer`` writes (trainer.py:169-170, :188) into ``model``, as the
    reference's dev / test modes do (main.py:23,36).  A file that does not hold this model's name is an error."""
    saved = torch.load(path, map_location=torch.device('cpu'))
    if not isinstance(saved, dict) or model.model_name not in saved:
        have = sorted(map(str, saved)) if isinstance(saved, dict) else type(saved).__name__
        raise KeyError(f"{path} holds no state dict for '{model.model_name}' (found: {have})")
    model.load_state_dict(saved[model.model_name])


def recommend_category(dc, max_per_category: int):
    """The per-news category array ``--recommend_max_per_category`` caps by, or None without a cap; a corpus that carries none
    cannot be capped."""
    if not max_per_category:
        return None
    category = getattr(dc, 'news_category', None)
    if category is None:
        raise ValueError('--recommend_max_per_category needs the category of every news, and this corpus carries none '
                         '(mind.load and synthetic.make_corpus give one: news_category)')
    return category


def recommend_lines(model, dc, k: int, batch_size: int, diversity=None, shortlist: int = 0, max_per_category: int = 0, calibration=None,
                    sample=None, seed: int = 0, rerank=None, exposure_cap=None):
    """``"<impression id> [id1,id2,...]"`` (1-based impression ids, best news first) for every impression of ``dc`` against the
    pool of all non-PAD news, the user's own history excluded; with ``diversity`` the diversified lists of ``util.recommend``, with
    ``calibration`` its calibrated ones, with ``sample`` (a temperature) one drawn slate per impression (``seed``), with ``rerank``
    (a pair) the jointly re-ranked ones, with ``exposure_cap`` the lists in which no news appears more often than that."""
    pool = torch.arange(1, dc.news_embedding.shape[0], dtype=torch.int64, device=dc.news_embedding.device)
    users = torch.arange(dc.history.shape[0], dtype=torch.int64)
    if exposure_cap is not None:
        ids, _, count = util.recommend(model, dc, users, pool, k, batch_size=batch_size, exposure_cap=exposure_cap, shortlist=shortlist or None)
    elif rerank is not None:
        ids, _, count = util.recommend(model, dc, users, pool, k, batch_size=batch_size, rerank=rerank, shortlist=shortlist or None,
                                       category=recommend_category(dc, max_per_category), max_per_category=max_per_category)
    elif sample is not None:
        ids, _, count = util.recommend(model, dc, users, pool, k, batch_size=batch_size, sample=sample, seed=seed, shortlist=shortlist or None)
    elif calibration is not None:
        ids, _, count = util.recommend(model, dc, users, pool, k, batch_size=batch_size, calibration=calibration, shortlist=shortlist or None)
    elif diversity is None:
        ids, _, count = util.recommend(model, dc, users, pool, k, batch_size=batch_size)
    else:
        ids, _, count = util.recommend(model, dc, users, pool, k, batch_size=batch_size, diversity=diversity, shortlist=shortlist or None,
                                       category=recommend_category(dc, max_per_category), max_per_category=max_per_category)
    ids, count = ids.cpu().numpy(), count.cpu().numpy()
    return ['%d [%s]' % (i + 1, ','.join(str(int(v)) for v in ids[i, :count[i]])) for i in range(len(count))]


def clicked_targets(dc, labels):
    """``(target_ids [T], target_start [I + 1])`` for all impressions of ``dc``: each impression's clicked candidates — the rows
    with label 1 — in row order (``nrms._clicked_targets`` reads the same for its corpus)."""
    imp, cand = dc.row_impression.cpu().numpy(), dc.row_candidate.cpu().numpy()
    rows = np.flatnonzero(np.asarray(labels) == 1)
    rows = rows[np.argsort(imp[rows], kind='stable')]
    start = np.r_[0, np.cumsum(np.bincount(imp[rows], minlength=int(dc.history.shape[0])))].astype(np.int64)
    return cand[rows].astype(np.int64), start


def report_lines(model, dc, k: int, batch_size: int, diversities, shortlist: int = 0, max_per_category: int = 0, labels=None):
    """One line per diversity of ``--recommend_report``: ``util.recommend_report`` for every impression of ``dc`` against the pool
    ``recommend_lines`` uses, ``evaluate.quality_summary``'s fields in its order; with ``labels`` (a labelled split) the accuracy
    fields against each impression's clicked candidates behind them."""
    pool = torch.arange(1, dc.news_embedding.shape[0], dtype=torch.int64, device=dc.news_embedding.device)
    users = torch.arange(dc.history.shape[0], dtype=torch.int64)
    rows = util.recommend_report(model, dc, users, pool, k, diversities, shortlist=shortlist or None,
                                 category=recommend_category(dc, max_per_category), max_per_category=max_per_category,
                                 targets=None if labels is None else clicked_targets(dc, labels), batch_size=batch_size)
    fmt = lambda v: '%d' % v if isinstance(v, int) else '%.4f' % v
    return ['diversity %.3f : ' % r['diversity'] + '  '.join('%s %s' % (f, fmt(v)) for f, v in r.items() if f != 'diversity') for r in rows]


def interval_lines(per_impression, replicates: int, level: float, seed: int):
    """One line per metric below the four of a labelled dev / test run: its bootstrap percentile interval over impressions
    (``evaluate.metric_intervals`` of the ``evaluate.impression_metrics`` rows), with the replicates, the level and the seed."""
    from . import evaluate
    got = evaluate.metric_intervals(per_impression, names=evaluate.METRIC_NAMES, replicates=replicates, level=level, seed=seed)
    label = dict(zip(evaluate.METRIC_NAMES, ('AUC', 'MRR', 'nDCG@5', 'nDCG@10')))
    return ['%s interval : [%.4f, %.4f]  se %.4f  (%d bootstrap replicates over %d impressions, level %g, seed %d)'
            % (label[k], v['lo'], v['hi'], v['se'], v['replicates'], int(per_impression.shape[0]), v['level'], seed) for k, v in got.items()]


def compare_lines(per_a, per_b, replicates: int, level: float, seed: int):
    """One line per metric of ``--compare_model_path``: the paired bootstrap of the two checkpoints' per-impression metrics
    (``evaluate.compare_metrics``; a is the scored model, b the compared one)."""
    from . import evaluate
    got = evaluate.compare_metrics(per_a, per_b, names=evaluate.METRIC_NAMES, replicates=replicates, level=level, seed=seed)
    label = dict(zip(evaluate.METRIC_NAMES, ('AUC', 'MRR', 'nDCG@5', 'nDCG@10')))
    return ['%s difference : %.4f - %.4f = %+.4f  [%+.4f, %+.4f]  se %.4f  p %.4f  wins %.3f  (%d paired replicates, level %g, seed %d)'
            % (label[k], v['a'], v['b'], v['diff'], v['lo'], v['hi'], v['se'], v['p'], v['wins'], replicates, level, seed)
            for k, v in got.items()]


def second_model(config, model, path: str, dev):
    """``--compare_model_path``: a model of the architecture of ``model`` (a table-backed news encoder shares the table's values)
    with the checkpoint at ``path`` loaded."""
    table = getattr(model.news_encoder, 'table', None)
    other = Model(config) if table is None else Model(config, news_encoder=PrecomputedNewsEncoder(table.detach().cpu().clone(), trainable=False))
    other.initialize()
    load_checkpoint(other, path)
    return other.to(dev)


def synthetic_setup(config, dev):
    """The synthetic corpus and a table-backed model: ``(model, dc, train corpus, labels of dc, dev_dc or None)``."""
    spec = synthetic.SynthSpec(news_num=config.synthetic_news, sag_neighbors=config.SAG_neighbors, sag_hops=config.SAG_hops,
                               max_history_num=config.max_history_num, category_num=config.category_num,
                               embedding_dim=config.news_embedding_dim, impressions=config.synthetic_impressions,
                               seed=config.seed)
    corpus = synthetic.make_corpus(spec)
    model = Model(config, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding),
                                                              trainable=config.mode == 'train'))
    model.initialize()
    if config.mode in ('dev', 'test', 'recommend'):
        load_checkpoint(model, config.dev_model_path if config.mode == 'dev' else config.test_model_path)
    model = model.to(dev)
    dc = util.DeviceCorpus.from_numpy(corpus, dev, user_graphs=config.user_graphs)
    return model, dc, corpus, corpus.row_label, None


def mind_setup(config, dev):
    """``--data_root``: the MIND files (``mind.load``) and the model with its text encoder.  ``train`` trains on the train split and
    selects on dev (one set of news tables for both: ``news_from``); ``dev`` scores the dev split, ``test`` and ``recommend`` the
    test split.  Returns what ``synthetic_setup`` returns; the labels are None for an unlabelled test file."""
    from . import mind
    corpus = mind.load(config.data_root, max_history_num=config.max_history_num, max_title_length=config.max_title_length,
                       word_threshold=config.word_threshold, sag_neighbors=config.SAG_neighbors, sag_hops=config.SAG_hops,
                       dataset=config.dataset, artefact_root=config.artefact_root or None, similarity_file=config.similarity_file or None,
                       word_embedding_file=config.word_embedding_file or None, word_embedding_dim=config.word_embedding_dim,
                       data_cache=config.data_cache or None, semantic_embedding_root=config.semantic_embedding_root or None, verbose=config.local_rank in (-1, 0))
    config.set_corpus(corpus)
    model = Model(config)
    model.initialize()
    if corpus.word_embedding is not None:
        weight = model.news_encoder.word_embedding.weight
        if tuple(corpus.word_embedding.shape) != tuple(weight.shape):
            raise ValueError(f"word embedding file holds {corpus.word_embedding.shape}, the model takes {tuple(weight.shape)}")
        with torch.no_grad():
            weight.copy_(torch.from_numpy(corpus.word_embedding))
    if config.mode in ('dev', 'test', 'recommend'):
        load_checkpoint(model, config.dev_model_path if config.mode == 'dev' else config.test_model_path)
    model = model.to(dev)
    if config.mode == 'train':
        dc = util.DeviceCorpus.from_numpy(corpus.train, dev, user_graphs=config.user_graphs)
        dev_dc = util.DeviceCorpus.from_numpy(corpus.dev, dev, user_graphs=config.user_graphs, news_from=dc)
        return model, dc, corpus.train, corpus.dev.row_label, dev_dc
    split = corpus.dev if config.mode == 'dev' else corpus.test
    return model, util.DeviceCorpus.from_numpy(split, dev, user_graphs=config.user_graphs), None, split.row_label, None


def main(argv=None):
    config = Config(argv)
    config.set_device()
    dev = torch.device('cuda', torch.cuda.current_device())
    on_mind = bool(getattr(config, 'data_root', ''))
    model, dc, corpus, labels, dev_dc = (mind_setup if on_mind else synthetic_setup)(config, dev)
    if config.mode == 'train':
        if config.train_input == 'device':
            from .train_input import DeviceTrainSet
            train_set = DeviceTrainSet(corpus, config.negative_sample_num, config.seed, dev)
        else:
            train_set = SyntheticTrainSet(corpus, config.negative_sample_num, config.seed)
        trainer = Trainer(model, config, dc, train_set, local_rank=config.local_rank, dev_labels=labels,
                          model_dir=getattr(config, 'model_dir', '') or None, dev_dc=dev_dc)
        trainer.train(max_steps=config.max_steps or None, log_every=50)
        if config.local_rank != -1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        if not trainer.is_main_rank:
            return
        if dev_dc is not None:
            dc = dev_dc                                              # the split the model was selected on
    if config.local_rank in (-1, 0):
        start = time.time()
        if hasattr(model.news_encoder, 'table'):                 # a text encoder's representations: compute_scores / recommend encode them
            dc.news_embedding = model.news_encoder.table.detach()
        if hasattr(model.graph_encoder, 'projection_mode'):      # the public switch of the scoring run's projection format
            model.graph_encoder.projection_mode = config.inference_projection
        if config.mode == 'recommend':
            diversity, cap = getattr(config, 'recommend_diversity', None), getattr(config, 'recommend_max_per_category', 0)
            calibration = getattr(config, 'recommend_calibration', None)
            recommend_category(dc, cap)                                     # refuse before the model runs
            rerank = getattr(config, 'recommend_rerank', None)
            if calibration is not None or (rerank is not None and rerank[1] != 0.0):
                util.calibration_category(None, getattr(dc, 'news_category', None))
            lines = recommend_lines(model, dc, config.recommend_k, config.batch_size * 16, diversity,
                                    getattr(config, 'recommend_shortlist', 0), cap, calibration,
                                    getattr(config, 'recommend_sample', None), getattr(config, 'recommend_seed', 0), rerank,
                                    getattr(config, 'recommend_exposure_cap', None))
            if config.recommend_output:
                with open(config.recommend_output, 'w') as f:
                    f.write('\n'.join(lines))
            print('Recommended %d news for each of %d impressions' % (config.recommend_k, len(lines)))
            if getattr(config, 'recommend_report', None):
                for line in report_lines(model, dc, config.recommend_k, config.batch_size * 16, config.recommend_report,
                                         getattr(config, 'recommend_shortlist', 0), cap, labels):
                    print(line)
            print('Inference time : %.1fs' % (time.time() - start))
            return
        result_file = config.test_output_file if config.mode == 'test' and config.test_output_file else None
        scores, metrics = util.compute_scores(model, dc, config.batch_size * 16, labels=labels, result_file=result_file)
        if metrics is not None:                                  # an unlabelled test file: the rank file is the result
            print('AUC : %.4f\nMRR : %.4f\nnDCG@5 : %.4f\nnDCG@10 : %.4f' % metrics)
        print('Inference time : %.1fs' % (time.time() - start))
        replicates = getattr(config, 'bootstrap', 0)
        if metrics is not None and replicates:                   # the instrument beside the means: percentile intervals over impressions
            from . import evaluate
            row_imp = dc.row_impression.cpu().numpy()
            per = evaluate.impression_metrics(torch.from_numpy(np.ascontiguousarray(scores)).to(dev), row_imp, labels)
            for line in interval_lines(per, replicates, config.bootstrap_level, config.seed):
                print(line)
            if config.compare_model_path:
                other = second_model(config, model, config.compare_model_path, dev)
                if hasattr(other.news_encoder, 'table'):
                    dc.news_embedding = other.news_encoder.table.detach()
                if hasattr(other.graph_encoder, 'projection_mode'):
                    other.graph_encoder.projection_mode = config.inference_projection
                scores_b, _ = util.compute_scores(other, dc, config.batch_size * 16)
                per_b = evaluate.impression_metrics(torch.from_numpy(np.ascontiguousarray(scores_b)).to(dev), row_imp, labels)
                for line in compare_lines(per, per_b, replicates, config.bootstrap_level, config.seed):
                    print(line)


if __name__ == '__main__':
    main()
