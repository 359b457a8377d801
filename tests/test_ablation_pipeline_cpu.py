"""CPU suite for the ablation encoders' scoring pipeline: the grouped entry exists on all five classes, the library exports the
device entries behind it under the unchanged ABI version, and ``main``'s loader reads the checkpoints ``Trainer`` writes
(no compute calls here)."""
import os
import types

import pytest
import torch

from oracle import digat_oracle as O


def _cfg(graph_encoder="DIGAT"):
    return types.SimpleNamespace(news_encoder="MSA", graph_encoder=graph_encoder, news_graph_size=4, max_history_num=10,
                                 category_num=5, graph_depth=2, dropout_rate=0.2)


@pytest.mark.parametrize("name", list(O.ABLATIONS))
def test_every_ablation_class_has_the_grouped_entry(name):
    import inspect
    from digat_amd import graphEncoders
    cls = getattr(graphEncoders, name)
    assert hasattr(cls, "inference_grouped"), name
    want = list(inspect.signature(graphEncoders.DIGAT.inference_grouped).parameters)[:10]       # self + the nine tensors
    sig = inspect.signature(cls.inference_grouped)
    assert list(sig.parameters)[:10] == want
    for kw in ("news_ctx_layers", "news_index"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default is None


def test_model_forwards_the_context_table_keyword():
    import inspect
    from digat_amd.model import Model
    assert "news_ctx_layers" in inspect.signature(Model.inference_grouped).parameters


def test_library_exports_the_grouped_context_entries():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    for n in ("digat_user_ctx_fwd_grouped", "digat_user_ctx_grouped_workspace_bytes", "digat_user_nodes_build"):
        assert hasattr(L, n) and n in _lib.EXPORTED, n
    assert L.digat_version() == _lib.ABI_VERSION == 4
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "digat_hip.h")).read()
    assert "#define DIGAT_ABI_VERSION 4" in header.replace("  ", " ")
    # the grouped workspace is the per-row entry's plus the per-row copies of the groups' indices, mask bytes and group index
    B, G, U, H, C1, d = 4096, 100, 67, 50, 18, 400
    base = L.digat_user_ctx_workspace_bytes(B, U, H, C1, d)
    got = L.digat_user_ctx_grouped_workspace_bytes(B, G, U, H, C1, d)
    assert base + B * (8 * H + C1 + 4) <= got <= base + B * (8 * H + C1 + 4) + 3 * 256
    # argument errors are answered on the host, before any launch: null row_group / no groups with rows to score
    one = torch.zeros(64)
    p = one.data_ptr()
    args = [p] * 3 + [None, p] + [p] * 8 + [None, p]
    assert L.digat_user_ctx_fwd_grouped(*args, 4, 2, 15, 10, 6, 64, p, 1 << 30, None) == 1                    # DIGAT_ERR_ARG
    args[3] = p
    assert L.digat_user_ctx_fwd_grouped(*args, 4, 0, 15, 10, 6, 64, p, 1 << 30, None) == 1
    assert L.digat_user_ctx_fwd_grouped(*args, 4, 2, 15, 10, 6, 62, p, 1 << 30, None) == 2                    # d % 4: DIGAT_ERR_SHAPE
    assert L.digat_user_ctx_fwd_grouped(*args, 4, 2, 15, 10, 6, 64, p, 16, None) == 3                         # DIGAT_ERR_WORKSPACE
    assert L.digat_user_ctx_fwd_grouped(*args, 0, 0, 15, 10, 6, 64, p, 1 << 30, None) == 0                    # B == 0: no launch
    assert L.digat_user_nodes_build(p, p, None, p, 0, 0, 10, 5, 64, None) == 0                                # rows == 0: no launch
    assert L.digat_user_nodes_build(p, p, None, p, 3, 2, 10, 5, 64, None) == 1                                # rows != G without a map


@pytest.mark.parametrize("choice", ["DIGAT", "wo_interaction"])
def test_main_loads_trainer_checkpoints(choice, tmp_path):
    from digat_amd import main as M
    from digat_amd.model import Model, PrecomputedNewsEncoder

    def make(seed):
        torch.manual_seed(seed)
        m = Model(_cfg(choice), news_encoder=PrecomputedNewsEncoder(torch.randn(8, 64)))
        m.initialize()
        with torch.no_grad():
            for p in m.parameters():           # biases and the topic nodes are zero-initialised: make every tensor tell the models apart
                p.add_(torch.randn_like(p) * 0.01)
        return m
    src, dst = make(1), make(2)
    assert src.model_name == "MSA-" + choice
    path = str(tmp_path / src.model_name)
    torch.save({src.model_name: src.state_dict()}, path)          # the format of trainer.Trainer (dev_epoch / train)
    assert any(not torch.equal(a, b) for a, b in zip(src.state_dict().values(), dst.state_dict().values()))
    M.load_checkpoint(dst, path)
    got, want = dst.state_dict(), src.state_dict()
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    other = str(tmp_path / "other")
    torch.save({"MSA-somebody_else": src.state_dict()}, other)
    with pytest.raises(KeyError, match=src.model_name):
        M.load_checkpoint(dst, other)


def test_config_has_the_model_path_flags():
    from digat_amd.config import Config
    c = Config(["--mode", "test", "--test_model_path", "a/b", "--dev_model_path", "c/d", "--test_output_file", "out.txt",
                "--graph_encoder", "wo_interaction"])
    assert (c.test_model_path, c.dev_model_path, c.test_output_file, c.graph_encoder) == ("a/b", "c/d", "out.txt", "wo_interaction")
    assert Config([]).test_output_file == ""
