"""Flags: the counterpart of the reference's ``config.py`` for the path this repo owns.

Same flag names, defaults and dataset overrides (config.py:14-75): MIND-small forces dropout 0.2 / 16 epochs,
MIND-large 0.1 / 7; ``news_graph_size = 1 + M + M(M-1) + ...``.  Differences, all forced by the environment:
real MIND cannot be downloaded, so the default corpus is synthetic (``--synthetic_news``, ``--synthetic_impressions``);
``--data_root`` names MIND files on disk instead (``mind.load``: ``--artefact_root``, ``--similarity_file``, ``--semantic_embedding_root``,
``--word_embedding_file``, ``--data_cache``, ``--word_threshold``, ``--max_title_length``), and only then are those flags attributes
(``--model_dir`` also when it is given: the Trainer saves there on either corpus);
``--recommend_diversity`` (with ``--recommend_shortlist``, ``--recommend_max_per_category``) likewise: attributes only when it is given;
``--recommend_report`` (a tuple of diversities; it brings the other two with it as well) likewise;
``--recommend_calibration`` (with ``--recommend_shortlist``, here up to 1024) likewise;
``--recommend_sample`` (a temperature; with ``--recommend_seed`` and ``--recommend_shortlist``, here up to 1024) likewise;
``--recommend_rerank`` (a pair ``D,C``; with ``--recommend_shortlist`` up to 1024 and ``--recommend_max_per_category``) likewise;
``--recommend_exposure_cap`` (a capacity per news over the lists of the call; with ``--recommend_shortlist`` up to 1024) likewise;
``--bootstrap`` (with ``--bootstrap_level``, ``--compare_model_path``) likewise;
``--local_rank`` also accepts torch >= 2.0's ``--local-rank`` spelling and the ``LOCAL_RANK`` variable.
"""
from __future__ import annotations

import argparse
import os
import random

import numpy as np
import torch

from .synthetic import news_graph_size


class Config:
    def __init__(self, argv=None):
        p = argparse.ArgumentParser(description='DIGAT (MI355X HIP path) experiments')
        p.add_argument('--mode', default='train', choices=['train', 'dev', 'test', 'recommend'])
        p.add_argument('--news_encoder', default='MSA', choices=['MSA', 'CNN'])
        p.add_argument('--graph_encoder', default='DIGAT',
                       choices=['DIGAT', 'wo_SA', 'Seq_SA', 'wo_interaction', 'news_graph_wo_inter', 'user_graph_wo_inter'])
        p.add_argument('--dev_model_path', type=str, default='best_model/MIND-small/MSA-DIGAT/#1/MSA-DIGAT', help='Dev model path')
        p.add_argument('--test_model_path', type=str, default='best_model/MIND-small/MSA-DIGAT/#1/MSA-DIGAT', help='Test model path')
        p.add_argument('--test_output_file', type=str, default='', help='Test output file (the rank file of --mode test)')
        p.add_argument('--recommend_k', type=int, default=10, help='news recommended per impression (--mode recommend; 1..128)')
        p.add_argument('--recommend_output', type=str, default='', help='Recommendation file of --mode recommend: "<impression id> [id1,id2,...]" per line')
        p.add_argument('--recommend_diversity', type=float, default=None,
                       help='--mode recommend: pick the k by maximal-marginal relevance from a shortlist, lam = 1 - this value (0..1; default: off)')
        p.add_argument('--recommend_shortlist', type=int, default=0,
                       help='the shortlist --recommend_diversity picks from (recommend_k..128; 0: min(128, 4 * recommend_k)); with '
                            '--recommend_calibration: recommend_k..1024; 0: min(1024, 8 * recommend_k)')
        p.add_argument('--recommend_max_per_category', type=int, default=0,
                       help='with --recommend_diversity: at most this many news of one category per list (0: no cap; needs a corpus with categories)')
        p.add_argument('--recommend_calibration', type=float, default=None,
                       help="--mode recommend: pick the k from a shortlist so that the list keeps the category mix of the reader's history, "
                            'lam = 1 - this value (0..1; default: off; needs a corpus with categories; not with --recommend_diversity)')
        p.add_argument('--recommend_sample', type=float, default=None,
                       help='--mode recommend: DRAW the k from a shortlist (recommend_k..1024; 0: min(1024, 8 * recommend_k)) — one Plackett-Luce '
                            'slate from softmax(score / this temperature) (> 0; default: off; not with --recommend_diversity, '
                            '--recommend_calibration or --recommend_report)')
        p.add_argument('--recommend_seed', type=int, default=0, help='with --recommend_sample: the seed of the draws')
        p.add_argument('--recommend_rerank', type=str, default=None,
                       help='--mode recommend: "D,C" — diversity and calibration at once, one greedy pass over a shortlist (recommend_k..1024; '
                            '0: min(1024, 8 * recommend_k)) with the weights 1 - D - C, D and C (each 0..1, D + C <= 1; default: off; honours '
                            '--recommend_max_per_category; not with --recommend_diversity, --recommend_calibration, --recommend_sample or '
                            '--recommend_report)')
        p.add_argument('--recommend_exposure_cap', type=int, default=None,
                       help='--mode recommend: no news in more than this many of the lists written (>= 0; default: off) — every list keeps its '
                            'best k of a shortlist (recommend_k..1024; 0: min(1024, 8 * recommend_k)) among the news that still have room for '
                            'it; not with --recommend_diversity, --recommend_calibration, --recommend_sample, --recommend_rerank, '
                            '--recommend_report or --recommend_max_per_category')
        p.add_argument('--recommend_report', type=str, default=None,
                       help='--mode recommend: diversities "0,0.1,0.3" to report list quality for (one scoring pass; honours --recommend_k, '
                            '--recommend_shortlist, --recommend_max_per_category)')
        p.add_argument('--bootstrap', type=int, default=0,
                       help='--mode dev|test on a labelled split: percentile intervals of the four metrics from this many bootstrap replicates '
                            'over impressions (0: none)')
        p.add_argument('--bootstrap_level', type=float, default=0.95, help='the level of the --bootstrap intervals')
        p.add_argument('--compare_model_path', type=str, default='',
                       help='with --bootstrap: a second checkpoint of the same architecture, compared with the first by a paired bootstrap')
        p.add_argument('--seed', type=int, default=0)
        p.add_argument('--local_rank', '--local-rank', type=int, default=int(os.environ.get('LOCAL_RANK', -1)))
        p.add_argument('--dataset', default='MIND-small', choices=['MIND-small', 'MIND-large'])
        p.add_argument('--negative_sample_num', type=int, default=4)
        p.add_argument('--max_history_num', type=int, default=50)
        p.add_argument('--epoch', type=int, default=16)
        p.add_argument('--batch_size', type=int, default=64)
        p.add_argument('--lr', type=float, default=1e-4)
        p.add_argument('--weight_decay', type=float, default=0)
        p.add_argument('--gradient_clip_norm', type=float, default=1)
        p.add_argument('--early_stopping_epoch', type=int, default=5)
        p.add_argument('--dev_criterion', default='avg', choices=['auc', 'mrr', 'ndcg5', 'ndcg10', 'avg'])
        p.add_argument('--train_precision', default='fp32', choices=['fp32', 'bf16'],
                       help='bf16: bf16 matrix-core operands for the large training GEMMs (fp32 master weights / accumulation)')
        p.add_argument('--dropout_rate', type=float, default=0.2)
        p.add_argument('--graph_depth', type=int, default=3)
        p.add_argument('--SAG_hops', type=int, default=2)
        p.add_argument('--SAG_neighbors', type=int, default=5)
        p.add_argument('--news_embedding_dim', type=int, default=400, help='MSA: 16 heads x 25')
        p.add_argument('--word_embedding_dim', type=int, default=300)
        p.add_argument('--cnn_method', default='naive', choices=['naive', 'group3', 'group4', 'group5'],
                       help='naive and group3 run; the others are refused by the encoder as the reference itself fails on them')
        p.add_argument('--cnn_kernel_num', type=int, default=400)
        p.add_argument('--cnn_window_size', type=int, default=3)
        p.add_argument('--attention_dim', type=int, default=256)
        p.add_argument('--MSA_head_num', type=int, default=16)
        p.add_argument('--MSA_head_dim', type=int, default=25)
        p.add_argument('--synthetic_news', type=int, default=8192)
        p.add_argument('--synthetic_impressions', type=int, default=2048)
        p.add_argument('--max_steps', type=int, default=0, help='stop training after this many steps (0 = all epochs)')
        p.add_argument('--inference_projection', default='auto',
                       choices=['auto', 'bf16x6', 'bf16x6-pq3', 'fp32', 'fp16x3', 'fp16-fp8c', 'pq-bf16', 'pq-bf16-x1', 'pq-fp8'],
                       help="the graph encoder's projection_mode for dev / test scoring (fp16-fp8c: fp16 + fp8 matrix-core corrections)")
        p.add_argument('--user_graphs', default='table', choices=['table', 'derived'],
                       help='table: user graphs uploaded with the corpus; derived: built on the device per batch from the category indices')
        p.add_argument('--train_input', default='host', choices=['host', 'device'],
                       help='host: negative sampling and batch indices in numpy; device: sampled per epoch and assembled per step by HIP kernels')
        # a MIND corpus on disk (mind.load): without --data_root none of these is an attribute and every path is the synthetic one
        p.add_argument('--data_root', type=str, default='', help='MIND files: train/, dev/ and test/, each with news.tsv and behaviors.tsv')
        p.add_argument('--artefact_root', type=str, default='',
                       help="directory of the reference's artefacts (news_ID-*.json ... news_graph-*.pkl): used where present")
        p.add_argument('--similarity_file', type=str, default='', help="the reference's similarity-M.json: news graphs by the device walk")
        p.add_argument('--semantic_embedding_root', type=str, default='',
                       help="the reference's <dataset>-SAG directory of sentence embeddings: similar-news lists and news graphs built on the device")
        p.add_argument('--word_embedding_file', type=str, default='', help="the reference's word_embedding-*.pkl or an .npy [V, dim]")
        p.add_argument('--data_cache', type=str, default='', help='directory the parsed corpus is cached in (rebuilt when stale)')
        p.add_argument('--word_threshold', type=int, default=3)
        p.add_argument('--max_title_length', type=int, default=32)
        p.add_argument('--model_dir', type=str, default='', help='directory the trained models are saved in')
        a = p.parse_args(argv)
        if a.recommend_report is not None:
            try:
                a.recommend_report = tuple(float(f) for f in a.recommend_report.split(',') if f.strip())
            except ValueError:
                p.error('--recommend_report takes diversities separated by commas, such as 0,0.1,0.3')
            if not a.recommend_report or not all(0.0 <= f <= 1.0 for f in a.recommend_report):
                p.error('--recommend_report needs at least one diversity, each in [0, 1]')
        if a.recommend_rerank is not None:
            try:
                a.recommend_rerank = tuple(float(f) for f in a.recommend_rerank.split(','))
            except ValueError:
                p.error('--recommend_rerank takes a diversity and a calibration separated by a comma, such as 0.2,0.4')
            if len(a.recommend_rerank) != 2 or not all(0.0 <= f <= 1.0 for f in a.recommend_rerank) or not sum(a.recommend_rerank) <= 1.0:
                p.error('--recommend_rerank needs two values D,C, each in [0, 1], with D + C <= 1')
            if (a.recommend_diversity is not None or a.recommend_calibration is not None or a.recommend_sample is not None
                    or a.recommend_report is not None):
                p.error('--recommend_rerank does not combine with --recommend_diversity, --recommend_calibration, --recommend_sample or '
                        '--recommend_report')
        if a.recommend_exposure_cap is not None:
            if a.recommend_exposure_cap < 0:
                p.error('--recommend_exposure_cap must not be negative')
            if (a.recommend_diversity is not None or a.recommend_calibration is not None or a.recommend_sample is not None
                    or a.recommend_rerank is not None or a.recommend_report is not None or a.recommend_max_per_category):
                p.error('--recommend_exposure_cap does not combine with --recommend_diversity, --recommend_calibration, --recommend_sample, '
                        '--recommend_rerank, --recommend_report or --recommend_max_per_category')
        if a.recommend_calibration is not None and not 0.0 <= a.recommend_calibration <= 1.0:
            p.error('--recommend_calibration must lie in [0, 1]')
        if a.recommend_calibration is not None and (a.recommend_diversity is not None or a.recommend_report is not None):
            p.error('--recommend_calibration does not combine with --recommend_diversity or --recommend_report')
        if a.recommend_sample is not None and not 0.0 < a.recommend_sample < float('inf'):
            p.error('--recommend_sample is a temperature: it must be positive and finite')
        if a.recommend_sample is not None and (a.recommend_diversity is not None or a.recommend_report is not None
                                               or a.recommend_calibration is not None or a.recommend_max_per_category):
            p.error('--recommend_sample does not combine with --recommend_diversity, --recommend_calibration, --recommend_report or '
                    '--recommend_max_per_category')
        if a.recommend_seed and a.recommend_sample is None:
            p.error('--recommend_seed needs --recommend_sample')
        if a.recommend_diversity is None and a.recommend_report is None and a.recommend_rerank is None and (
                a.recommend_max_per_category or (a.recommend_shortlist and a.recommend_calibration is None and a.recommend_sample is None
                                                 and a.recommend_exposure_cap is None)):
            p.error('--recommend_shortlist and --recommend_max_per_category need --recommend_diversity (0 for the cap alone) or --recommend_report')
        if a.recommend_diversity is not None and not 0.0 <= a.recommend_diversity <= 1.0:
            p.error('--recommend_diversity must lie in [0, 1]')
        if a.recommend_shortlist < 0 or a.recommend_max_per_category < 0:
            p.error('--recommend_shortlist and --recommend_max_per_category must not be negative')
        if a.bootstrap < 0 or not 0.0 < a.bootstrap_level < 1.0:
            p.error('--bootstrap must not be negative and --bootstrap_level must lie inside (0, 1)')
        if a.compare_model_path and not a.bootstrap:
            p.error('--compare_model_path needs --bootstrap B: the replicates of the paired bootstrap')
        mind_flags = ('data_root', 'artefact_root', 'similarity_file', 'semantic_embedding_root', 'word_embedding_file', 'data_cache', 'word_threshold',
                      'max_title_length', 'model_dir')
        diversity_flags = ('recommend_diversity', 'recommend_shortlist', 'recommend_max_per_category')    # attributes only when asked for
        report_flags = ('recommend_report', 'recommend_shortlist', 'recommend_max_per_category')
        calibration_flags = ('recommend_calibration', 'recommend_shortlist')
        sample_flags = ('recommend_sample', 'recommend_seed', 'recommend_shortlist')
        rerank_flags = ('recommend_rerank', 'recommend_shortlist', 'recommend_max_per_category')
        exposure_flags = ('recommend_exposure_cap', 'recommend_shortlist')
        bootstrap_flags = ('bootstrap', 'bootstrap_level', 'compare_model_path')
        asked = lambda k: ((a.recommend_diversity is not None and k in diversity_flags) or (a.recommend_report is not None and k in report_flags)
                           or (a.recommend_calibration is not None and k in calibration_flags) or (a.bootstrap and k in bootstrap_flags)
                           or (a.recommend_sample is not None and k in sample_flags)
                           or (a.recommend_rerank is not None and k in rerank_flags)
                           or (a.recommend_exposure_cap is not None and k in exposure_flags)
                           or k not in diversity_flags + report_flags + calibration_flags + sample_flags + rerank_flags + exposure_flags
                           + bootstrap_flags)
        self.attribute_dict = {k: v for k, v in vars(a).items()
                               if (a.data_root or k not in mind_flags or (k == 'model_dir' and a.model_dir)) and asked(k)}
        for k, v in self.attribute_dict.items():
            setattr(self, k, v)
        if self.dataset == 'MIND-small':
            self.dropout_rate, self.epoch, self.category_num = 0.2, 16, 17
        else:
            self.dropout_rate, self.epoch, self.category_num = 0.1, 7, 18
        self.news_graph_size = news_graph_size(self.SAG_neighbors, self.SAG_hops)
        if not a.data_root:
            self.max_title_length = 1                               # synthetic "titles" are news ids

    def set_corpus(self, corpus):
        """The sizes a MIND corpus decides (MIND_corpus.py:192-204)."""
        self.user_num, self.category_num = corpus.user_num, corpus.category_num
        self.subCategory_num, self.vocabulary_size = corpus.subCategory_num, corpus.vocabulary_size

    def set_device(self):
        assert torch.cuda.is_available(), 'GPU is not available'
        if self.local_rank == -1:
            torch.cuda.set_device(0)
        else:
            import datetime
            import torch.distributed as dist
            torch.cuda.set_device(self.local_rank)
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            dist.init_process_group(backend='nccl', timeout=datetime.timedelta(0, 43200))   # RCCL on ROCm
        torch.manual_seed(self.seed)
        random.seed(self.seed)
        np.random.seed(self.seed)
