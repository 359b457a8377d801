"""MIND corpus loader: ``news.tsv`` / ``behaviors.tsv`` (and the reference's json / pkl artefacts) -> the arrays the device entries take.

The counterpart of the reference's ``MIND_corpus.py`` (``preprocess`` :24-108, ``__init__`` :189-321) in numpy and the standard
library: no torchtext, no sentence-transformers, no import of the reference.  What it produces has the attribute names of
``synthetic.SynthCorpus``, so ``util.DeviceCorpus.from_numpy``, ``train_input.behavior_arrays``, ``trainer.SyntheticTrainSet`` and
``train_input.DeviceTrainSet`` take a ``MindSplit`` unchanged.

* dictionaries (:36-87): ``user_ID`` (``<UNK>`` 0, training users), ``news_ID`` (``<PAD>`` 0; train, dev, test files in that order,
  first occurrence), ``category``, ``subCategory``, ``word_dict`` (``<PAD>`` 0, ``<UNK>`` 1).  Titles are lower-cased, ``é`` -> ``e``,
  cut by ``[\\w]+|[.,!?;|]``; what ``float()`` accepts counts as ``<NUM>``; words of the dev / test news count only if training has
  seen them; a stable sort by descending count, then ``word_threshold``.
* news arrays (:241-266): ``news_title_text`` [news_num, Lw] int32, ``news_title_mask`` bool, ``news_category`` [news_num] int64.
* per split: ``history`` [I, H] int32 (the last H read, right-padded with 0), ``user_category_indices`` [I, H] int64 (padding C),
  ``user_category_mask`` [I, C+1] bool, and one row per (impression, candidate): ``row_impression`` / ``row_candidate`` /
  ``row_label`` (``None`` for a behaviours file whose candidates carry no ``-0`` / ``-1`` suffix: MIND-large's test set, :313-314).
  The ``[I, U, U]`` user graphs are never built on the host: ``DeviceCorpus.from_numpy`` derives them from the indices on the device
  (``digat_user_graph_build``), as a table or per batch.
* news graphs, first source that exists: the reference's ``news_graph-<hops>-<M>-<dataset>.pkl`` (``mask[:, 0] = 0``, :210); a
  similarity file ``{news_ID: [[news_ID, cos], ...]}`` walked on the device (``construct_SAG.generate_news_graph`` ->
  ``digat_sag_news_graph``), then ``+ I`` and the cleared mask column (:118, :210); a directory of sentence embeddings in the
  reference's layout (``semantic_embedding_root``: ``construct_SAG.build_similarity`` makes the similar-news lists on the device, the
  same walk follows); else singleton graphs (node 0 only) with a notice.

Departures from the reference, all documented here:
* a title number (``<NUM>``) that falls under ``word_threshold`` is absent from ``word_dict``; the reference raises ``KeyError`` at
  :260, this loader maps it to ``<UNK>``;
* the training behaviours stay ``train_input.behavior_arrays``'s: a click whose impression has no non-clicked news is skipped (the
  reference keeps it, and its sampler then divides by zero, MIND_dataset.py:36);
* labelled or not is read off each behaviours file (every candidate ends in ``-0`` / ``-1``, or none does), not off ``--dataset``;
* a news that several files list takes its category from the first file (MIND's files agree).
"""
from __future__ import annotations

import glob
import json
import os
import pickle
import re
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np

from .synthetic import news_graph_size

_PAT = re.compile(r"[\w]+|[.,!?;|]")
SPLITS = ("train", "dev", "test")
CACHE_VERSION = 2


def is_number(s: str) -> bool:
    """MIND_corpus.py:12-17: whatever ``float()`` parses (so also ``nan``, ``inf`` and ``1_000``)."""
    try:
        float(s)
        return True
    except ValueError:
        return False


def tokenize(title: str):
    return _PAT.findall(title.lower().replace('é', 'e'))


# --------------------------------------------------------------------------------------------------------------------------------
# files
# --------------------------------------------------------------------------------------------------------------------------------
def read_news(roots):
    """The unique news of the three ``news.tsv`` in file order: ``(news_ID, category, subCategory, title, file index)``."""
    seen, out = set(), []
    for i, root in enumerate(roots):
        with open(os.path.join(root, 'news.tsv'), 'r', encoding='utf-8') as f:
            for line in f:
                if not line.strip():
                    continue
                news_ID, category, subCategory, title = line.split('\t')[:4]
                if news_ID not in seen:
                    seen.add(news_ID)
                    out.append((news_ID, category, subCategory, title, i))
    return out


def read_news_text(roots):
    """``read_news`` with the abstract, which the SAG's sentence embeddings are made of too:
    ``(news_ID, category, subCategory, title, abstract, file index)``."""
    seen, out = set(), []
    for i, root in enumerate(roots):
        with open(os.path.join(root, 'news.tsv'), 'r', encoding='utf-8') as f:
            for line in f:
                if not line.strip():
                    continue
                news_ID, category, subCategory, title, abstract = line.split('\t')[:5]
                if news_ID not in seen:
                    seen.add(news_ID)
                    out.append((news_ID, category, subCategory, title, abstract, i))
    return out


def build_dictionaries(news, train_root: str, word_threshold: int) -> Dict[str, dict]:
    """MIND_corpus.py:36-87 over ``read_news``'s list."""
    user_ID = {'<UNK>': 0}
    with open(os.path.join(train_root, 'behaviors.tsv'), 'r', encoding='utf-8') as f:
        for line in f:
            user = line.split('\t', 2)[1]
            if user not in user_ID:
                user_ID[user] = len(user_ID)
    news_ID, category, subCategory = {'<PAD>': 0}, {}, {}
    counter: Dict[str, int] = {}
    for nid, cat, sub, title, i in news:
        news_ID[nid] = len(news_ID)
        if cat not in category:
            category[cat] = len(category)
        if sub not in subCategory:
            subCategory[sub] = len(subCategory)
        for word in tokenize(title):
            if is_number(word):
                counter['<NUM>'] = counter.get('<NUM>', 0) + 1
            elif i == 0 or word in counter:          # dev / test words count only if training has seen them
                counter[word] = counter.get(word, 0) + 1
    ordered = sorted(counter.items(), key=lambda x: x[1], reverse=True)          # stable: equal counts keep first-seen order
    word_dict = {'<PAD>': 0, '<UNK>': 1}
    for word, count in ordered:
        if count >= word_threshold:
            word_dict[word] = len(word_dict)
    return {'user_ID': user_ID, 'news_ID': news_ID, 'category': category, 'subCategory': subCategory, 'word_dict': word_dict}


def _artefact(root: str, prefix: str, suffix: str, dataset: str) -> Optional[str]:
    """``<root>/<prefix><dataset><suffix>``, or the only file ``<prefix>*<suffix>`` there; None when there is none."""
    exact = os.path.join(root, prefix + dataset + suffix)
    if os.path.exists(exact):
        return exact
    found = sorted(glob.glob(os.path.join(glob.escape(root), prefix + '*' + suffix)))
    if len(found) > 1:
        raise ValueError(f"{root}: several files match {prefix}*{suffix}; name the dataset")
    return found[0] if found else None


def load_artefact_dictionaries(root: str, dataset: str, word_threshold: int, max_title_length: int) -> Optional[Dict[str, dict]]:
    """The five dictionaries the reference's ``preprocess`` wrote, or None unless all five are there."""
    names = {'user_ID': 'user_ID-', 'news_ID': 'news_ID-', 'category': 'category-', 'subCategory': 'subCategory-',
             'word_dict': 'vocabulary-%d-%d-' % (word_threshold, max_title_length)}
    paths = {k: _artefact(root, p, '.json', dataset) for k, p in names.items()}
    if any(p is None for p in paths.values()):
        return None
    out = {}
    for k, p in paths.items():
        with open(p, 'r', encoding='utf-8') as f:
            out[k] = json.load(f)
    return out


def load_word_embedding(path: str) -> np.ndarray:
    """``[V, dim]`` float32 from an ``.npy`` or from the reference's pickled tensor (``word_embedding-*.pkl``, :107-108)."""
    if path.endswith('.npy'):
        table = np.load(path)
    else:
        import torch  # noqa: F401  (the pickle holds a torch tensor)
        with open(path, 'rb') as f:
            table = pickle.load(f)
        table = table.detach().cpu().numpy() if hasattr(table, 'detach') else np.asarray(table)
    if table.ndim != 2:
        raise ValueError(f"{path}: a word embedding is [vocabulary_size, dim], got {table.shape}")
    return np.ascontiguousarray(table, dtype=np.float32)


# --------------------------------------------------------------------------------------------------------------------------------
# corpus
# --------------------------------------------------------------------------------------------------------------------------------
@dataclass
class MindSplit:
    """One behaviours file against the shared news side, with ``synthetic.SynthCorpus``'s attribute names."""
    corpus: "MindCorpus"
    name: str
    history: np.ndarray                      # [I, H] int32
    user_category_indices: np.ndarray        # [I, H] int64, padding = C
    user_category_mask: np.ndarray           # [I, C+1] bool
    row_impression: np.ndarray               # [R] int64
    row_candidate: np.ndarray                # [R] int32
    row_label: Optional[np.ndarray]          # [R] int8, or None: an unlabelled file
    user_graph = None                        # never on the host: derived from the indices on the device
    news_embedding = None                    # the text encoder's output: computed on the device

    @property
    def spec(self):
        c = self.corpus
        return SimpleNamespace(news_num=c.news_num, category_num=c.category_num, max_history_num=c.params['max_history_num'],
                               sag_neighbors=c.params['sag_neighbors'], sag_hops=c.params['sag_hops'],
                               news_graph_size=c.news_graph_size, user_graph_size=c.params['max_history_num'] + c.category_num,
                               impressions=int(self.history.shape[0]))

    @property
    def rows(self) -> int:
        return int(self.row_impression.shape[0])

    @property
    def user_graph_mask(self) -> np.ndarray:
        """[I, U] bool: live history slots and present topic nodes (MIND_corpus.py:167-168)."""
        C = self.corpus.category_num
        return np.concatenate([self.user_category_indices != C, self.user_category_mask[:, :C]], axis=1)

    # the shared news side
    news_category = property(lambda self: self.corpus.news_category)
    news_title_text = property(lambda self: self.corpus.news_title_text)
    news_title_mask = property(lambda self: self.corpus.news_title_mask)
    news_node_ID = property(lambda self: self.corpus.graphs()[0])
    news_graph = property(lambda self: self.corpus.graphs()[1])
    news_graph_mask = property(lambda self: self.corpus.graphs()[2])


@dataclass
class MindCorpus:
    params: dict                             # the loader parameters the arrays depend on
    dictionaries: Dict[str, dict]            # user_ID, news_ID, category, subCategory, word_dict
    news_title_text: np.ndarray              # [news_num, Lw] int32
    news_title_mask: np.ndarray              # [news_num, Lw] bool
    news_category: np.ndarray                # [news_num] int64 (row 0, <PAD>: 0)
    news_subCategory: np.ndarray             # [news_num] int64
    splits: Dict[str, MindSplit] = field(default_factory=dict)
    news_node_ID: Optional[np.ndarray] = None        # [news_num, N] int32
    news_graph: Optional[np.ndarray] = None          # [news_num, N, N] bool
    news_graph_mask: Optional[np.ndarray] = None     # [news_num, N] bool, column 0 cleared
    news_graph_source: str = ""                      # "artefact", "similarity", "embeddings" or "singleton"
    similarity: Optional[dict] = None                # a similarity file read but not walked yet
    embedding_news: Optional[list] = None            # read_news_text's list: the SAG is built from params['semantic_embedding_root'] on first use
    word_embedding: Optional[np.ndarray] = None      # [V, dim] float32, or None: the module's own initialisation
    tsv_sizes: dict = field(default_factory=dict)

    news_num = property(lambda self: len(self.dictionaries['news_ID']))
    category_num = property(lambda self: len(self.dictionaries['category']))
    subCategory_num = property(lambda self: len(self.dictionaries['subCategory']))
    user_num = property(lambda self: len(self.dictionaries['user_ID']))
    vocabulary_size = property(lambda self: len(self.dictionaries['word_dict']))
    news_graph_size = property(lambda self: news_graph_size(self.params['sag_neighbors'], self.params['sag_hops']))
    train = property(lambda self: self.splits['train'])
    dev = property(lambda self: self.splits['dev'])
    test = property(lambda self: self.splits['test'])

    def graphs(self):
        """(news_node_ID, news_graph, news_graph_mask); a similarity file is walked here, on the device, on first use, and so are
        the lists built from sentence embeddings."""
        if self.news_graph is None:
            if self.similarity is not None:
                self.set_news_graphs(*walk_similarity(self.similarity, self.dictionaries['news_ID'], self.params['sag_neighbors'],
                                                      self.params['sag_hops'], self.news_graph_size), source="similarity")
            elif self.embedding_news is not None:
                self.set_news_graphs(*walk_embeddings(self.embedding_news, self.dictionaries, self.params['semantic_embedding_root'],
                                                      self.params['sag_neighbors'], self.params['sag_hops'], self.news_graph_size,
                                                      self.params['dataset']), source="embeddings")
            else:
                raise ValueError("this corpus has no news graphs")
            self.similarity = self.embedding_news = None
        return self.news_node_ID, self.news_graph, self.news_graph_mask

    def set_news_graphs(self, node_ID, graph, mask, source: str):
        N = self.news_graph_size
        if node_ID.shape != (self.news_num, N) or graph.shape != (self.news_num, N, N) or mask.shape != (self.news_num, N):
            raise ValueError(f"news graphs of {graph.shape[0]} news and {graph.shape[1:]} nodes; the corpus has {self.news_num} news "
                             f"and news_graph_size {N}")
        self.news_node_ID = np.ascontiguousarray(node_ID, dtype=np.int32)
        self.news_graph = np.ascontiguousarray(graph, dtype=bool)
        self.news_graph_mask = np.array(mask, dtype=bool)
        self.news_graph_mask[:, 0] = False                                        # MIND_corpus.py:210
        self.news_graph_source = source

    # ---- cache: one .npz per split and for the news side, the dictionaries as json, a header that names what they were built from
    def header(self) -> dict:
        return {'version': CACHE_VERSION, 'params': self.params, 'tsv_sizes': self.tsv_sizes}

    def save(self, directory: str) -> None:
        self.graphs()
        os.makedirs(directory, exist_ok=True)
        news = dict(news_title_text=self.news_title_text, news_title_mask=self.news_title_mask, news_category=self.news_category,
                    news_subCategory=self.news_subCategory, news_node_ID=self.news_node_ID, news_graph=self.news_graph,
                    news_graph_mask=self.news_graph_mask, news_graph_source=np.array(self.news_graph_source))
        if self.word_embedding is not None:
            news['word_embedding'] = self.word_embedding
        np.savez(os.path.join(directory, 'news.npz'), **news)
        for name, s in self.splits.items():
            arrays = dict(history=s.history, user_category_indices=s.user_category_indices, user_category_mask=s.user_category_mask,
                          row_impression=s.row_impression, row_candidate=s.row_candidate)
            if s.row_label is not None:
                arrays['row_label'] = s.row_label
            np.savez(os.path.join(directory, name + '.npz'), **arrays)
        with open(os.path.join(directory, 'dictionaries.json'), 'w', encoding='utf-8') as f:
            json.dump(self.dictionaries, f)
        with open(os.path.join(directory, 'header.json'), 'w', encoding='utf-8') as f:        # last: a cache without it is no cache
            json.dump(self.header(), f)

    @classmethod
    def load(cls, directory: str) -> "MindCorpus":
        with open(os.path.join(directory, 'header.json'), 'r', encoding='utf-8') as f:
            header = json.load(f)
        if header.get('version') != CACHE_VERSION:
            raise ValueError(f"{directory}: cache version {header.get('version')}, this loader writes {CACHE_VERSION}")
        with open(os.path.join(directory, 'dictionaries.json'), 'r', encoding='utf-8') as f:
            dictionaries = json.load(f)
        with np.load(os.path.join(directory, 'news.npz')) as z:
            corpus = cls(header['params'], dictionaries, z['news_title_text'], z['news_title_mask'], z['news_category'],
                         z['news_subCategory'], news_node_ID=z['news_node_ID'], news_graph=z['news_graph'],
                         news_graph_mask=z['news_graph_mask'], news_graph_source=str(z['news_graph_source']),
                         word_embedding=z['word_embedding'] if 'word_embedding' in z.files else None, tsv_sizes=header['tsv_sizes'])
        for name in SPLITS:
            with np.load(os.path.join(directory, name + '.npz')) as z:
                corpus.splits[name] = MindSplit(corpus, name, z['history'], z['user_category_indices'], z['user_category_mask'],
                                                z['row_impression'], z['row_candidate'], z['row_label'] if 'row_label' in z.files else None)
        return corpus


def walk_similarity(similarity: dict, news_ID: dict, top_M: int, hops: int, node_num: int):
    """Similarity lists -> (news_node_ID, news_graph + I, news_graph_mask) through the device walk (there is no host walk here)."""
    from . import construct_SAG
    lists = {nid: similarity.get(nid, []) for nid in news_ID}                      # a news the file does not list has no neighbours
    for nid, entries in lists.items():
        for other, _ in entries:
            if other not in news_ID:
                raise ValueError(f"similarity list of {nid} names {other}, which is no news of the corpus")
    node_ID, graph, mask = construct_SAG.generate_news_graph(None, lists, news_ID, top_M, hops, node_num)
    graph = graph | np.identity(node_num, dtype=bool)[None]                        # MIND_corpus.py:118
    return node_ID, graph, mask


def walk_embeddings(news, dictionaries: dict, embedding_root: str, top_M: int, hops: int, node_num: int, dataset: str):
    """Sentence embeddings -> similar-news lists -> (news_node_ID, news_graph + I, news_graph_mask), all on the device."""
    import torch
    from . import construct_SAG
    lists = construct_SAG.build_similarity(news, dictionaries, embedding_root, top_M, dataset)
    node_ID, graph, mask = construct_SAG.news_graph_device(*lists, top_M=top_M, hop=hops, news_node_num=node_num)
    graph = graph | torch.eye(node_num, dtype=torch.bool, device=graph.device)[None]          # MIND_corpus.py:118
    return node_ID.cpu().numpy(), graph.cpu().numpy(), mask.cpu().numpy()


def singleton_graphs(news_num: int, node_num: int):
    """Every news alone in its graph: node 0 is the news, identity adjacency, empty mask — what an isolated news gets from the walk."""
    node_ID = np.zeros((news_num, node_num), dtype=np.int32)
    node_ID[1:, 0] = np.arange(1, news_num, dtype=np.int32)
    graph = np.broadcast_to(np.identity(node_num, dtype=bool), (news_num, node_num, node_num)).copy()
    return node_ID, graph, np.zeros((news_num, node_num), dtype=bool)


def parse_behaviors(path: str, news_ID: dict, news_category: np.ndarray, category_num: int, max_history_num: int,
                    corpus: MindCorpus, name: str) -> MindSplit:
    """One ``behaviors.tsv`` -> a ``MindSplit`` (MIND_corpus.py:145-176 for the category arrays, :269-321 for histories and rows)."""
    H, C = max_history_num, category_num
    hist_rows, hist_len, cand, label, per_imp = [], [], [], [], []
    labelled = None
    with open(path, 'r', encoding='utf-8') as f:
        for line_no, line in enumerate(f):
            _, _, _, history, impressions = line.split('\t')
            try:
                read = [news_ID[x] for x in history.split(' ')] if history.strip() else []
                read = read[-H:]
                hist_len.append(len(read))
                hist_rows.append(read + [0] * (H - len(read)))
                tokens = impressions.strip().split(' ')
                suffixed = [t[-2:] in ('-0', '-1') for t in tokens]
                if labelled is None:
                    labelled = suffixed[0]
                if any(s != labelled for s in suffixed):
                    raise ValueError(f"{path}:{line_no + 1}: labelled and unlabelled candidates in one file")
                if labelled:
                    cand.extend(news_ID[t[:-2]] for t in tokens)
                    label.extend(t[-1] == '1' for t in tokens)
                else:
                    cand.extend(news_ID[t] for t in tokens)
            except KeyError as e:
                raise ValueError(f"{path}:{line_no + 1}: news {e} is in no news.tsv / news_ID dictionary") from None
            per_imp.append(len(tokens))
    I = len(per_imp)
    history = np.asarray(hist_rows, dtype=np.int32).reshape(I, H)
    valid = np.arange(H)[None, :] < np.asarray(hist_len, dtype=np.int64).reshape(I, 1)
    cat_idx = np.where(valid, news_category[history], C).astype(np.int64)
    cat_mask = np.zeros((I, C + 1), dtype=bool)
    rows, cols = np.nonzero(valid)
    cat_mask[rows, cat_idx[rows, cols]] = True
    return MindSplit(corpus, name, history, cat_idx, cat_mask, np.repeat(np.arange(I, dtype=np.int64), np.asarray(per_imp, dtype=np.int64)),
                     np.asarray(cand, dtype=np.int32), np.asarray(label, dtype=np.int8) if labelled else None)


def _embedding_files(root: Optional[str]):
    if not root:
        return ()
    return tuple(sorted(p for sub in ('semantic_embeddings', 'corpus_semantic_embeddings') for ext in ('pkl', 'npy')
                        for p in glob.glob(os.path.join(glob.escape(root), sub, '*_semantic_embeddings-*.' + ext))))


def _tsv_sizes(roots, extra=()):
    files = [os.path.join(r, n) for r in roots for n in ('news.tsv', 'behaviors.tsv')] + [p for p in extra if p]
    return {p: os.path.getsize(p) for p in files}


def load(data_root: str, max_history_num: int = 50, max_title_length: int = 32, word_threshold: int = 3, sag_neighbors: int = 5,
         sag_hops: int = 2, dataset: str = 'MIND-small', artefact_root: Optional[str] = None, similarity_file: Optional[str] = None,
         word_embedding_file: Optional[str] = None, word_embedding_dim: int = 300, data_cache: Optional[str] = None,
         defer_news_graphs: bool = False, verbose: bool = True, semantic_embedding_root: Optional[str] = None) -> MindCorpus:
    """The corpus under ``data_root`` (``train/``, ``dev/``, ``test/``, each with ``news.tsv`` and ``behaviors.tsv``).

    ``artefact_root``: a directory of the reference's artefacts; its five dictionaries are used instead of being rebuilt when all
    are there (the news count is checked against the files, :251), its ``news_graph`` / ``word_embedding`` pkl are taken, and the
    category indices of its ``user_history_graph`` pkl are checked against the loader's.  ``similarity_file``: walked on the device
    unless the artefacts hold the news graphs — at once, or with ``defer_news_graphs`` on first use (nothing is cached then: the
    cache holds the graphs).  ``semantic_embedding_root``: the reference's ``<dataset>-SAG`` directory of sentence embeddings
    (``construct_SAG.read_embeddings``); with neither graphs nor a similarity file the similar-news lists are built from it on the
    device and walked, at once or deferred as a similarity file is.  ``data_cache``: a directory
    ``MindCorpus.save`` wrote is loaded when its header names these parameters and these files' sizes, and (re)written otherwise."""
    roots = [os.path.join(data_root, s) for s in SPLITS]
    params = dict(max_history_num=int(max_history_num), max_title_length=int(max_title_length), word_threshold=int(word_threshold),
                  sag_neighbors=int(sag_neighbors), sag_hops=int(sag_hops), dataset=dataset, artefact_root=artefact_root,
                  similarity_file=similarity_file, word_embedding_file=word_embedding_file, word_embedding_dim=int(word_embedding_dim),
                  semantic_embedding_root=semantic_embedding_root)
    sizes = _tsv_sizes(roots, (similarity_file, word_embedding_file) + _embedding_files(semantic_embedding_root))
    if data_cache and os.path.exists(os.path.join(data_cache, 'header.json')):
        with open(os.path.join(data_cache, 'header.json'), 'r', encoding='utf-8') as f:
            header = json.load(f)
        if header == {'version': CACHE_VERSION, 'params': params, 'tsv_sizes': sizes}:
            return MindCorpus.load(data_cache)
        if verbose:
            print(f"mind: the cache in {data_cache} was built from other files or parameters; rebuilding it", flush=True)

    news = read_news(roots)
    dictionaries = load_artefact_dictionaries(artefact_root, dataset, word_threshold, max_title_length) if artefact_root else None
    if dictionaries is None:
        dictionaries = build_dictionaries(news, roots[0], word_threshold)
    news_ID, word_dict, category, subCategory = (dictionaries[k] for k in ('news_ID', 'word_dict', 'category', 'subCategory'))
    if len(news_ID) != len(news) + 1:                                            # MIND_corpus.py:251
        raise ValueError('news num mismatch %d v.s. %d' % (len(news_ID), len(news)))
    news_num, Lw = len(news_ID), int(max_title_length)
    text = np.zeros((news_num, Lw), dtype=np.int32)
    mask = np.zeros((news_num, Lw), dtype=bool)
    news_category = np.zeros(news_num, dtype=np.int64)
    news_sub = np.zeros(news_num, dtype=np.int64)
    unk, num = word_dict['<UNK>'], word_dict.get('<NUM>', word_dict['<UNK>'])    # <NUM> under the threshold: <UNK> (the reference raises)
    for nid, cat, sub, title, _ in news:
        try:
            index = news_ID[nid]
            news_category[index], news_sub[index] = category[cat], subCategory[sub]
        except KeyError as e:
            raise ValueError(f"{e} of news {nid} is missing from the dictionaries") from None
        words = tokenize(title)[:Lw]
        text[index, :len(words)] = [num if is_number(w) else word_dict.get(w, unk) for w in words]
        mask[index, :len(words)] = True
    corpus = MindCorpus(params, dictionaries, text, mask, news_category, news_sub, tsv_sizes=sizes)
    for name, root in zip(SPLITS, roots):
        corpus.splits[name] = parse_behaviors(os.path.join(root, 'behaviors.tsv'), news_ID, news_category, len(category),
                                              int(max_history_num), corpus, name)

    graph_file = _artefact(artefact_root, 'news_graph-%d-%d-' % (sag_hops, sag_neighbors), '.pkl', dataset) if artefact_root else None
    if graph_file:
        with open(graph_file, 'rb') as f:
            g = pickle.load(f)
        corpus.set_news_graphs(g['news_node_ID'], g['news_graph'], g['news_graph_mask'], source="artefact")
    elif similarity_file:
        with open(similarity_file, 'r', encoding='utf-8') as f:
            corpus.similarity = json.load(f)
        if not defer_news_graphs:
            corpus.graphs()
    elif semantic_embedding_root:
        corpus.embedding_news = read_news_text(roots)
        if not defer_news_graphs:
            corpus.graphs()
    else:
        if verbose:
            print("mind: no news_graph artefact, no similarity file and no sentence embeddings: every news graph is the news alone", flush=True)
        corpus.set_news_graphs(*singleton_graphs(news_num, corpus.news_graph_size), source="singleton")
    if artefact_root:
        user_file = _artefact(artefact_root, 'user_history_graph-%d-' % max_history_num, '.pkl', dataset)
        if user_file:
            with open(user_file, 'rb') as f:
                u = pickle.load(f)
            for name in SPLITS:
                theirs = u.get(name + '_user_history_category_indices')
                if theirs is not None and not np.array_equal(theirs, corpus.splits[name].user_category_indices):
                    raise ValueError(f"{user_file}: the {name} category indices differ from the ones read off {roots[SPLITS.index(name)]}")
    if word_embedding_file is None and artefact_root:
        word_embedding_file = _artefact(artefact_root, 'word_embedding-%d-%d-%d-' % (word_threshold, word_embedding_dim, Lw), '.pkl', dataset)
    if word_embedding_file:
        corpus.word_embedding = load_word_embedding(word_embedding_file)
        if corpus.word_embedding.shape[0] != len(word_dict):
            raise ValueError(f"{word_embedding_file}: {corpus.word_embedding.shape[0]} rows for a vocabulary of {len(word_dict)}")
    elif verbose:
        print("mind: no word embedding file: the word embedding keeps the module's own initialisation", flush=True)
    if verbose:
        print(f"mind: news graphs from {corpus.news_graph_source or 'a source walked on first use'}", flush=True)
    if data_cache and (corpus.news_graph is not None or corpus.similarity is not None or corpus.embedding_news is not None):
        if not (defer_news_graphs and corpus.news_graph is None):
            corpus.save(data_cache)
    return corpus
