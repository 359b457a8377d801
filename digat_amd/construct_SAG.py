"""Semantic-augmented-graph construction on the GPU: the reference's construct_SAG.py from sentence embeddings
to news graphs.

``generate_cos_similarities`` (construct_SAG.py:112-162) and ``generate_news_graph`` (:449-485) keep the reference's
names, argument order and return values; both run on ``cuda:0`` through the C ABI (``digat_sag_cos_topk``,
``digat_sag_news_graph``) and there is no CPU path.  The steps between them run here too:

* ``news_meta`` restates the news bookkeeping of ``generate_semantic_embeddings`` (:13-92) for one category: the title groups, the
  texts to embed in row order, the news with no text at all;
* ``similar_news_lists_device`` (``digat_sag_similar_lists``) is ``generate_similariy_info`` + ``generate_similar_news_list`` +
  ``aggregate`` (:217-446) for the one kind ``aggregate`` reads, the average: cosine GEMM, selection and the per-news walk over the
  k best corpus groups in one call per category, writing the ``[news_num, top_M]`` arrays ``news_graph_device`` takes.  No
  per-kind tables, dictionaries or JSON files in between.  ``similar_news_lists_host`` is its numpy yardstick;
* ``build_similarity`` is the driver over the categories (:560-567), ``semantic_augmented_news`` Appendix B's table
  (MIND_corpus.py:113-119), ``write_similarity_json`` the reference's ``similarity-M.json``.

Only the sentence-transformer itself (:93-109) stays outside: embeddings are read from the reference's layout
(``<root>/semantic_embeddings/{title,content}_semantic_embeddings-<category>.pkl`` or ``.npy``, ``<root>/corpus_semantic_embeddings/``
for the corpus side); ``python -m digat_amd.construct_SAG meta`` writes the texts to embed, in row order.

Departures from the reference, all documented here:
* a news with neither title nor abstract gets random same-category neighbours with cosine 0 (:386-400).  The reference draws them
  with an unseeded ``np.random.choice``; here ``np.random.default_rng(seed)`` draws ``top_M + 1`` distinct positions of the
  category's news list (all of them when it is shorter), skips the news itself and keeps at most ``top_M``.  Real MIND has
  essentially no such news;
* :32 leaves the test news out of the corpus side when ``dataset_type == 'small'``, but the reference's ``MIND_corpus.py`` hands it
  ``'MIND-small'``, so there the exclusion never fires.  ``excludes_test`` takes both spellings as the small dataset.
"""
from __future__ import annotations

import json
import os
import pickle
from typing import Dict, Sequence

import numpy as np
import torch

from . import _lib

similarity_threshold = 0.5          # construct_SAG.py:10
_MAX_K = 32


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.DigatHipError("digat_amd.construct_SAG runs on the GPU only; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def cos_topk_device(title: torch.Tensor, content: torch.Tensor, corpus_title: torch.Tensor, corpus_content: torch.Tensor,
                    top_M: int):
    """Device tensors in, device tensors out: (values [5, n, k] f32, indices [5, n, k] int32), k = min(top_M, m - 1) + 1;
    kinds in the order ``generate_cos_similarities`` returns them."""
    dev = _lib.require_device(title, content, corpus_title, corpus_content)
    title, content, corpus_title, corpus_content = (_lib.f32(t) for t in (title, content, corpus_title, corpus_content))
    n, dim = title.shape
    m = corpus_title.shape[0]
    if content.shape != (n, dim) or corpus_title.shape != (m, dim) or corpus_content.shape != (m, dim):
        raise ValueError("title/content must be [n, dim] and the corpus embeddings [m, dim]")
    if m < 1:
        raise ValueError("empty corpus")
    k = min(top_M, m - 1) + 1                                            # :115
    if k > _MAX_K:
        raise ValueError(f"top_M + 1 = {k} exceeds the kernel's limit of {_MAX_K}")
    L = _lib.lib()
    values = torch.empty((5, n, k), dtype=torch.float32, device=dev)
    indices = torch.empty((5, n, k), dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.digat_sag_cos_topk_workspace_bytes(n, m, dim), dev, "sag")
    _lib.check(L.digat_sag_cos_topk(title.data_ptr(), content.data_ptr(), n, corpus_title.data_ptr(), corpus_content.data_ptr(), m,
                                    dim, k, values.data_ptr(), indices.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "digat_sag_cos_topk")
    return values, indices


def generate_cos_similarities(dataset_type, top_M, category, title_semantic_embeddings, content_semantic_embeddings,
                              corpus_title_semantic_embeddings, corpus_content_semantic_embeddings):
    """construct_SAG.py:112-233 without the pickle cache (``dataset_type`` / ``category`` only name the reference's cache
    files and are ignored): ten CPU tensors, (values [n, k] f32, indices [n, k] int32) for title, content, title-content,
    content-title and average, each row as ``torch.topk`` returns it."""
    dev = _device()
    args = [torch.as_tensor(t, dtype=torch.float32).to(dev) for t in
            (title_semantic_embeddings, content_semantic_embeddings, corpus_title_semantic_embeddings, corpus_content_semantic_embeddings)]
    values, indices = cos_topk_device(*args, top_M=top_M)
    values, indices = values.cpu(), indices.cpu()
    out = []
    for kind in range(5):
        out += [values[kind], indices[kind]]
    return tuple(out)


def similarity_lists(news_similarity_dict: Dict[str, Sequence], news_ID_dict: Dict[str, int], top_M: int):
    """{news_ID: [[news_ID, cos], ...]} (``aggregate``, :425-446) -> (sim_index [num, top_M] int32, sim_cos f32, sim_len int32)
    indexed by ``news_ID_dict`` value."""
    news_num = len(news_ID_dict)
    sim_index = np.zeros((news_num, top_M), dtype=np.int32)
    sim_cos = np.zeros((news_num, top_M), dtype=np.float32)
    sim_len = np.zeros(news_num, dtype=np.int32)
    for news_ID, row in news_ID_dict.items():
        entries = news_similarity_dict[news_ID]
        if len(entries) > top_M:
            raise ValueError(f"{news_ID}: {len(entries)} similar news, more than top_M = {top_M}")
        sim_len[row] = len(entries)
        for e, (other, cos) in enumerate(entries):
            sim_index[row, e] = news_ID_dict[other]
            sim_cos[row, e] = cos
    return sim_index, sim_cos, sim_len


def news_graph_device(sim_index: torch.Tensor, sim_cos: torch.Tensor, sim_len: torch.Tensor, top_M: int, hop: int,
                      news_node_num: int, threshold: float = similarity_threshold):
    """Device arrays in, device tensors out: (news_node_ID int32 [num, nn], news_graph bool [num, nn, nn], mask bool [num, nn])."""
    dev = _lib.require_device(sim_index, sim_cos, sim_len)
    num = sim_len.shape[0]
    if sim_index.dtype != torch.int32 or sim_len.dtype != torch.int32 or sim_cos.dtype != torch.float32:
        raise ValueError("sim_index / sim_len must be int32 and sim_cos float32")
    if tuple(sim_index.shape) != (num, top_M) or tuple(sim_cos.shape) != (num, top_M):
        raise ValueError("sim_index / sim_cos must be [news_num, top_M]")
    sim_index, sim_cos, sim_len = sim_index.contiguous(), sim_cos.contiguous(), sim_len.contiguous()
    node_ID = torch.empty((num, news_node_num), dtype=torch.int32, device=dev)
    graph = torch.empty((num, news_node_num, news_node_num), dtype=torch.uint8, device=dev)
    mask = torch.empty((num, news_node_num), dtype=torch.uint8, device=dev)
    overflow = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().digat_sag_news_graph(sim_index.data_ptr(), sim_cos.data_ptr(), sim_len.data_ptr(), num, top_M, hop,
                                               news_node_num, float(threshold), node_ID.data_ptr(), graph.data_ptr(),
                                               mask.data_ptr(), overflow.data_ptr(), _lib.stream_ptr()),
               "digat_sag_news_graph")
    if int(overflow.item()):
        raise IndexError("a news graph needs more than news_node_num nodes")      # the reference's numpy IndexError at :474
    return node_ID, graph.view(torch.bool), mask.view(torch.bool)


def generate_news_graph(dataset_type, news_similarity_dict, news_ID_dict, top_M, hop, news_node_num):
    """construct_SAG.py:449-485: (news_node_ID int32 [num, nn], news_graph bool [num, nn, nn], news_graph_mask bool [num, nn])
    as numpy arrays (``dataset_type`` is unused there too)."""
    dev = _device()
    arrays = similarity_lists(news_similarity_dict, news_ID_dict, top_M)
    node_ID, graph, mask = news_graph_device(*(torch.from_numpy(a).to(dev) for a in arrays), top_M=top_M, hop=hop,
                                             news_node_num=news_node_num)
    return node_ID.cpu().numpy(), graph.cpu().numpy(), mask.cpu().numpy()


# --------------------------------------------------------------------------------------------------------------------------------
# embeddings -> similar-news lists
# --------------------------------------------------------------------------------------------------------------------------------
def excludes_test(dataset: str) -> bool:
    """construct_SAG.py:32: the small dataset keeps its test news out of the corpus side (see the module header)."""
    return dataset in ('small', 'MIND-small')


def news_meta(news_rows, mode: str, corpus_excludes_test: bool):
    """construct_SAG.py:13-92 for one category.  ``news_rows``: ``(data_domain, news_ID, title, abstract)`` in file order,
    ``data_domain`` ``'train_dev'`` or ``'test'``.  Returns the reference's five items: ``news_dict`` {news_ID: group},
    ``news_dict_inv`` {str(group): [news_ID]}, ``titles`` and ``contents`` (the texts to embed, one per group) and
    ``empty_news_IDs``."""
    if mode not in ('corpus', 'full'):
        raise ValueError("mode is 'corpus' or 'full'")
    members: Dict[str, list] = {}                # title -> its news, groups in first-seen order
    content_of: Dict[str, str] = {}
    empty_news_IDs, seen = [], set()
    for data_domain, news_ID, title, content in news_rows:
        if mode == 'corpus' and corpus_excludes_test and data_domain == 'test':
            continue
        if news_ID in seen:
            continue
        seen.add(news_ID)
        title, content = title.lower().replace('é', 'e'), content.lower().replace('é', 'e')
        if title == '' and content == '':
            empty_news_IDs.append(news_ID)
            continue
        if title == '':
            title = content
        elif content == '':
            content = title
        content_of[news_ID] = content
        members.setdefault(title, []).append(news_ID)
    news_dict, news_dict_inv, titles, contents = {}, {}, [], []
    for i, (title, ids) in enumerate(members.items()):
        titles.append(title)
        contents.append(next((content_of[x] for x in ids if content_of[x] != ''), title))      # the first non-empty content
        news_dict_inv[str(i)] = list(ids)
        for news_ID in ids:
            news_dict[news_ID] = i
    count: Dict[str, int] = {}
    for content in contents:
        count[content] = count.get(content, 0) + 1
    contents = [titles[i] + ' ' + c if count[c] > 1 else c for i, c in enumerate(contents)]      # duplicated contents: title first
    return news_dict, news_dict_inv, titles, contents, empty_news_IDs


def category_rows(news):
    """``mind.read_news_text``'s list -> {category: [(data_domain, news_ID, title, abstract)]} in file order (the reference's
    ``<dataset>-SAG/news/<category>.tsv``, :535-550) and the categories that have train / dev news (``non_empty_corpus``)."""
    rows: Dict[str, list] = {}
    has_corpus = set()
    for news_ID, category, _, title, abstract, file_index in news:
        rows.setdefault(category, []).append(('train_dev' if file_index < 2 else 'test', news_ID, title, abstract))
        if file_index < 2:
            has_corpus.add(category)
    return rows, has_corpus


def group_csr(news_dict_inv: Dict[str, Sequence[str]], news_ID_dict: Dict[str, int]):
    """``news_dict_inv`` -> (start [groups + 1] int32, member int32): the news rows of every group, in its order."""
    start, member = [0], []
    for g in range(len(news_dict_inv)):
        member.extend(news_ID_dict[x] for x in news_dict_inv[str(g)])
        start.append(len(member))
    return np.asarray(start, dtype=np.int32), np.asarray(member, dtype=np.int32)


def validate_csr(start, member, groups: int, news_num: int, what: str, nonempty: bool = False) -> None:
    """A CSR table the lists kernel indexes with: ``start`` [groups + 1] monotone from 0 to ``len(member)``, every member a news row
    in ``[1, news_num)``, no row twice (every news row has one writer), and — the corpus side — no empty group."""
    start, member = np.asarray(start), np.asarray(member)
    if start.ndim != 1 or member.ndim != 1 or start.shape[0] != groups + 1:
        raise ValueError(f"{what}: start must be [{groups + 1}], member one-dimensional")
    if int(start[0]) != 0 or int(start[-1]) != member.shape[0]:
        raise ValueError(f"{what}: start runs from {int(start[0])} to {int(start[-1])}, the member table has {member.shape[0]} rows")
    steps = np.diff(start.astype(np.int64))
    if (steps < 0).any():
        raise ValueError(f"{what}: start is not monotone")
    if nonempty and (steps == 0).any():
        raise ValueError(f"{what}: an empty group")
    if member.size and (int(member.min()) < 1 or int(member.max()) >= news_num):
        raise ValueError(f"{what}: member rows must lie in [1, {news_num}), got [{int(member.min())}, {int(member.max())}]")
    if np.unique(member).size != member.size:
        raise ValueError(f"{what}: a news row is listed twice")


def similar_news_lists_host(values, indices, k: int, group_start, group_member, corpus_start, corpus_member, top_M: int,
                            news_num: int, out=None):
    """The numpy yardstick of ``digat_sag_similar_lists``: ``values`` / ``indices`` [n, k] are the average top-k of every query
    group (corpus GROUP indices), ``k = M' + 1``.  Restates construct_SAG.py:304-320 on arrays: every member news of a group walks
    the k entries in order, skips a corpus group that holds the news itself, takes (first member of the corpus group, cosine) and
    stops once M' are taken — with M' = 0 the stop test never fires.  Writes into ``out`` = (sim_index, sim_cos, sim_len) when
    given, else into fresh zero arrays ``[news_num, top_M]`` / ``[news_num]``; rows of news in no group are not touched."""
    values, indices = np.asarray(values, dtype=np.float32), np.asarray(indices)
    sim_index, sim_cos, sim_len = out if out is not None else (np.zeros((news_num, top_M), dtype=np.int32),
                                                               np.zeros((news_num, top_M), dtype=np.float32),
                                                               np.zeros(news_num, dtype=np.int32))
    stop = k - 1
    for g in range(len(group_start) - 1):
        for x in group_member[group_start[g]:group_start[g + 1]]:
            cnt = 0
            for e in range(k):
                c = int(indices[g, e])
                group = corpus_member[corpus_start[c]:corpus_start[c + 1]]
                if x in group:
                    continue
                sim_index[x, cnt], sim_cos[x, cnt] = group[0], values[g, e]
                cnt += 1
                if cnt == stop:
                    break
            sim_len[x] = cnt
    return sim_index, sim_cos, sim_len


def similar_news_lists_device(title: torch.Tensor, content: torch.Tensor, corpus_title: torch.Tensor, corpus_content: torch.Tensor,
                              top_M: int, group_start, group_member, corpus_start, corpus_member, news_num: int, out=None):
    """One category through ``digat_sag_similar_lists`` on the current stream.  Device embeddings in; the CSR tables are host arrays
    (numpy or CPU tensors), validated here — a bad table is a ``ValueError``, never a store past the arrays — and uploaded.  Writes
    rows of ``out`` = device (sim_index int32 [news_num, top_M], sim_cos f32, sim_len int32 [news_num]), or of fresh zero arrays."""
    n, m = int(title.shape[0]), int(corpus_title.shape[0])
    tables = [np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.int32)
              for t in (group_start, group_member, corpus_start, corpus_member)]
    if top_M < 1 or news_num < 1:
        raise ValueError("top_M and news_num must be positive")
    validate_csr(tables[0], tables[1], n, news_num, "query groups")
    validate_csr(tables[2], tables[3], m, news_num, "corpus groups", nonempty=True)
    dev = _lib.require_device(title, content, corpus_title, corpus_content)
    title, content, corpus_title, corpus_content = (_lib.f32(t) for t in (title, content, corpus_title, corpus_content))
    dim = title.shape[1]
    if content.shape != (n, dim) or corpus_title.shape != (m, dim) or corpus_content.shape != (m, dim):
        raise ValueError("title/content must be [n, dim] and the corpus embeddings [m, dim]")
    if m < 1:
        raise ValueError("empty corpus")
    if min(top_M, m - 1) + 1 > _MAX_K:
        raise ValueError(f"top_M + 1 = {min(top_M, m - 1) + 1} exceeds the kernel's limit of {_MAX_K}")
    if out is None:
        out = (torch.zeros((news_num, top_M), dtype=torch.int32, device=dev), torch.zeros((news_num, top_M), dtype=torch.float32, device=dev),
               torch.zeros(news_num, dtype=torch.int32, device=dev))
    sim_index, sim_cos, sim_len = out
    _lib.require_device(title, sim_index, sim_cos, sim_len)
    if (sim_index.dtype, sim_cos.dtype, sim_len.dtype) != (torch.int32, torch.float32, torch.int32) or not all(t.is_contiguous() for t in out):
        raise ValueError("sim_index / sim_len must be contiguous int32 and sim_cos contiguous float32")
    if tuple(sim_index.shape) != (news_num, top_M) or tuple(sim_cos.shape) != (news_num, top_M) or tuple(sim_len.shape) != (news_num,):
        raise ValueError("sim_index / sim_cos must be [news_num, top_M] and sim_len [news_num]")
    gs, gm, cs, cm = (torch.from_numpy(t).to(dev) for t in tables)
    L = _lib.lib()
    ws = _lib.workspace(L.digat_sag_similar_lists_workspace_bytes(n, m, dim), dev, "sag")
    _lib.check(L.digat_sag_similar_lists(title.data_ptr(), content.data_ptr(), n, corpus_title.data_ptr(), corpus_content.data_ptr(), m, dim,
                                         top_M, gs.data_ptr(), gm.data_ptr(), cs.data_ptr(), cm.data_ptr(), sim_index.data_ptr(),
                                         sim_cos.data_ptr(), sim_len.data_ptr(), news_num, ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "digat_sag_similar_lists")
    return sim_index, sim_cos, sim_len


EMBEDDING_DIRS = {'full': 'semantic_embeddings', 'corpus': 'corpus_semantic_embeddings'}


def read_embeddings(embedding_root: str, mode: str, category: str, rows: int):
    """(title, content) float32 [rows, dim] of one category and mode from the reference's layout: the pickled tensor (:100-103) or
    an ``.npy`` of the same stem.  Another row count than ``news_meta``'s is a ``ValueError``."""
    out = []
    for kind in ('title', 'content'):
        stem = os.path.join(embedding_root, EMBEDDING_DIRS[mode], '%s_semantic_embeddings-%s' % (kind, category))
        if os.path.exists(stem + '.pkl'):
            path = stem + '.pkl'
            with open(path, 'rb') as f:
                table = pickle.load(f)
            table = table.detach().cpu().numpy() if hasattr(table, 'detach') else np.asarray(table)
        elif os.path.exists(stem + '.npy'):
            path = stem + '.npy'
            table = np.load(path)
        else:
            raise FileNotFoundError(f"{stem}.pkl / .npy: no {kind} embeddings of category '{category}'")
        if table.ndim != 2 or table.shape[0] != rows:
            raise ValueError(f"{path}: {table.shape[0] if table.ndim else 0} rows, news_meta gives {rows} texts for this category")
        out.append(np.ascontiguousarray(table, dtype=np.float32))
    if out[0].shape != out[1].shape:
        raise ValueError(f"{stem}: title embeddings {out[0].shape}, content embeddings {out[1].shape}")
    return out


def empty_news_lists(rng, empty_news_IDs, candidates, news_ID_dict, top_M: int):
    """construct_SAG.py:386-400 with a seeded generator (see the module header): [(news row, [neighbour rows])]."""
    out = []
    for news_ID in empty_news_IDs:
        draw = rng.choice(len(candidates), size=min(top_M + 1, len(candidates)), replace=False)
        picked = [candidates[p] for p in draw if candidates[p] != news_ID][:top_M]
        out.append((news_ID_dict[news_ID], [news_ID_dict[x] for x in picked]))
    return out


def category_tables(rows, news_ID_dict, dataset: str):
    """One category's two ``news_meta`` and their CSR tables: (full meta, corpus meta, group_start, group_member, corpus_start,
    corpus_member)."""
    full = news_meta(rows, 'full', excludes_test(dataset))
    corpus = news_meta(rows, 'corpus', excludes_test(dataset))
    return (full, corpus) + group_csr(full[1], news_ID_dict) + group_csr(corpus[1], news_ID_dict)


def build_similarity(news, dictionaries, embedding_root: str, top_M: int, dataset: str, seed: int = 0):
    """The driver over all categories (construct_SAG.py:560-567) -> device (sim_index [news_num, top_M] int32, sim_cos f32,
    sim_len [news_num] int32), ready for ``news_graph_device``.  ``news``: ``mind.read_news_text``'s list; ``dictionaries``: the
    loader's (``news_ID``, ``category``).  A category with no train / dev news is skipped and its news keep empty lists, as
    ``aggregate`` gives them.  One ``similar_news_lists_device`` call per category on the current stream, all into one set of arrays."""
    dev = _device()
    news_ID_dict = dictionaries['news_ID']
    news_num = len(news_ID_dict)
    out = (torch.zeros((news_num, top_M), dtype=torch.int32, device=dev), torch.zeros((news_num, top_M), dtype=torch.float32, device=dev),
           torch.zeros(news_num, dtype=torch.int32, device=dev))
    rows, has_corpus = category_rows(news)
    rng = np.random.default_rng(seed)
    drawn = []
    for category in dictionaries['category']:
        if category not in has_corpus:
            continue
        full, corpus, gs, gm, cs, cm = category_tables(rows[category], news_ID_dict, dataset)
        tables = read_embeddings(embedding_root, 'full', category, len(full[2])) + read_embeddings(embedding_root, 'corpus', category, len(corpus[2]))
        if len(full[2]):
            similar_news_lists_device(*(torch.from_numpy(t).to(dev) for t in tables), top_M, gs, gm, cs, cm, news_num, out=out)
        drawn += empty_news_lists(rng, full[4], [r[1] for r in rows[category]], news_ID_dict, top_M)
    if drawn:                                        # the few news with no text: written from the host, cosine 0
        idx = np.zeros((len(drawn), top_M), dtype=np.int32)
        for r, (_, picked) in enumerate(drawn):
            idx[r, :len(picked)] = picked
        at = torch.tensor([x for x, _ in drawn], dtype=torch.int64, device=dev)
        out[0][at] = torch.from_numpy(idx).to(dev)
        out[1][at] = 0.0
        out[2][at] = torch.tensor([len(p) for _, p in drawn], dtype=torch.int32, device=dev)
    return out


def semantic_augmented_news(sim_index, sim_len, augmented_news_num: int):
    """Appendix B's table (MIND_corpus.py:113-119): [news_num, A] int32, the first A entries of each list, zero-padded, row 0 zero.
    Tensors (any device) or numpy arrays in, the same kind out."""
    A = int(augmented_news_num)
    if isinstance(sim_index, torch.Tensor):
        take = min(A, sim_index.shape[1])
        out = torch.zeros((sim_index.shape[0], A), dtype=torch.int32, device=sim_index.device)
        live = torch.arange(take, device=sim_index.device)[None, :] < sim_len[:, None]
        out[:, :take] = torch.where(live, sim_index[:, :take], torch.zeros_like(sim_index[:, :take]))
        out[0] = 0
        return out
    take = min(A, sim_index.shape[1])
    out = np.zeros((sim_index.shape[0], A), dtype=np.int32)
    out[:, :take] = np.where(np.arange(take)[None, :] < np.asarray(sim_len)[:, None], sim_index[:, :take], 0)
    out[0] = 0
    return out


def similarity_dict(sim_index, sim_cos, sim_len, news_ID_dict: Dict[str, int]) -> Dict[str, list]:
    """The arrays as ``aggregate``'s dictionary {news_ID: [[news_ID, cos], ...]}, every news a key."""
    sim_index, sim_cos, sim_len = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (sim_index, sim_cos, sim_len))
    name = {row: news_ID for news_ID, row in news_ID_dict.items()}
    return {news_ID: [[name[int(sim_index[row, e])], float(sim_cos[row, e])] for e in range(int(sim_len[row]))]
            for news_ID, row in news_ID_dict.items()}


def write_similarity_json(path: str, sim_index, sim_cos, sim_len, news_ID_dict: Dict[str, int]) -> None:
    """The reference's ``similarity-M.json`` (:441-442); ``similarity_lists`` reads it back to the same arrays (a float32 cosine
    survives the round trip through its shortest double)."""
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(similarity_dict(sim_index, sim_cos, sim_len, news_ID_dict), f)


def write_news_meta(news, embedding_root: str, dataset: str) -> list:
    """``news_meta-<category>.json`` of every category with train / dev news and both modes, in the reference's layout (:77-84):
    ``titles`` and ``contents`` are the texts to embed, in row order.  Returns the files written."""
    rows, has_corpus = category_rows(news)
    written = []
    for category in rows:
        if category not in has_corpus:
            continue
        for mode, sub in EMBEDDING_DIRS.items():
            meta = news_meta(rows[category], mode, excludes_test(dataset))
            os.makedirs(os.path.join(embedding_root, sub), exist_ok=True)
            path = os.path.join(embedding_root, sub, 'news_meta-%s.json' % category)
            with open(path, 'w', encoding='utf-8') as f:
                json.dump(dict(zip(('news_dict', 'news_dict_inv', 'titles', 'contents', 'empty_news_IDs'), meta)), f)
            written.append(path)
    return written


def main(argv=None):
    """``python -m digat_amd.construct_SAG {meta,build} --data_root ... --embedding_root ... --top_M ... --dataset ...``"""
    import argparse
    from . import mind
    p = argparse.ArgumentParser(prog='python -m digat_amd.construct_SAG', description=main.__doc__)
    p.add_argument('command', choices=['meta', 'build'],
                   help='meta: write news_meta-<category>.json (the texts to embed); build: embeddings -> similarity-M.json')
    p.add_argument('--data_root', required=True, help='MIND files: train/, dev/ and test/, each with news.tsv')
    p.add_argument('--embedding_root', required=True, help="the reference's <dataset>-SAG directory")
    p.add_argument('--top_M', type=int, default=5)
    p.add_argument('--dataset', default='MIND-small')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--output', default='', help='build: the file to write (default <embedding_root>/similarity-<top_M>.json)')
    a = p.parse_args(argv)
    news = mind.read_news_text([os.path.join(a.data_root, s) for s in mind.SPLITS])
    if a.command == 'meta':
        for path in write_news_meta(news, a.embedding_root, a.dataset):
            print(path)
        return
    news_ID = {'<PAD>': 0}
    category = {}
    for row in news:
        news_ID[row[0]] = len(news_ID)
        category.setdefault(row[1], len(category))
    arrays = build_similarity(news, {'news_ID': news_ID, 'category': category}, a.embedding_root, a.top_M, a.dataset, seed=a.seed)
    output = a.output or os.path.join(a.embedding_root, 'similarity-%d.json' % a.top_M)
    write_similarity_json(output, *arrays, news_ID)
    print(output)


if __name__ == '__main__':
    main()
