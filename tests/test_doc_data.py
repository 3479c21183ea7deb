"""Document masking from the token file to the trainers: the dataset yields
each window's layout, the config validates, and every trainer without
document-masked attention refuses instead of training unmasked."""
import dataclasses

import pytest
import torch

from trainingjob_operator_amd.launcher.data import (
    TokenFileDataset, make_batches, write_token_file,
)
from trainingjob_operator_amd.ops.docmask import (
    check_doc_bounds, doc_bounds_from_eos,
)
from trainingjob_operator_amd.training import TrainConfig

EOS = 5


@pytest.fixture(scope="module")
def token_file(tmp_path_factory):
    g = torch.Generator().manual_seed(3)
    toks = torch.randint(0, 40, (4096,), generator=g).tolist()
    return write_token_file(
        str(tmp_path_factory.mktemp("docdata") / "tokens.bin"), toks)


def test_dataset_with_eos_yields_bounds_of_its_tokens(token_file):
    ds = TokenFileDataset(token_file, seq_len=128, micro_batch=3,
                          eos_token=EOS)
    it = ds.batches()
    seen_cut = False
    for _ in range(3):
        batch = next(it)
        assert len(batch) == 3
        tokens, targets, bounds = batch
        assert tokens.shape == targets.shape == (3, 128)
        assert bounds.dtype == torch.int32 and bounds.shape == (2, 3, 128)
        assert bounds.device == tokens.device
        check_doc_bounds(bounds)
        assert torch.equal(bounds, doc_bounds_from_eos(tokens, EOS))
        # a document ends exactly where the tokens hold eos (or the window
        # ends)
        idx = torch.arange(128).expand(3, 128)
        ends = bounds[1] == idx
        assert torch.equal(ends[:, :-1], (tokens == EOS)[:, :-1])
        assert bool(ends[:, -1].all())
        seen_cut |= bool((bounds[0] > 0).any())
    assert seen_cut


def test_dataset_without_eos_is_unchanged(token_file):
    plain = TokenFileDataset(token_file, seq_len=128, micro_batch=2)
    with_eos = TokenFileDataset(token_file, seq_len=128, micro_batch=2,
                                eos_token=EOS)
    a, b = next(plain.batches()), next(with_eos.batches())
    assert len(a) == 2
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_make_batches_follows_the_config(token_file):
    base = TrainConfig(model="llama-tiny", micro_batch=2, seq_len=64,
                       data_path=token_file)
    assert len(next(make_batches(base, None))) == 2
    # an eos token alone does not switch the mask on
    cfg = dataclasses.replace(base, eos_token=EOS)
    assert len(next(make_batches(cfg, None))) == 2
    cfg = dataclasses.replace(base, eos_token=EOS, doc_mask=True)
    tokens, _, bounds = next(make_batches(cfg, None))
    assert torch.equal(bounds, doc_bounds_from_eos(tokens, EOS))


def test_train_config_validation(token_file):
    TrainConfig(doc_mask=True, data_path=token_file, eos_token=0)
    with pytest.raises(ValueError, match="data_path"):
        TrainConfig(doc_mask=True, eos_token=EOS)              # synthetic
    with pytest.raises(ValueError, match="eos_token"):
        TrainConfig(doc_mask=True, data_path=token_file)       # eos -1
    with pytest.raises(ValueError, match="use_graphs"):
        TrainConfig(doc_mask=True, data_path=token_file, eos_token=EOS,
                    use_graphs=True)
    # unset, nothing is asked of the other fields
    TrainConfig(use_graphs=True)
    TrainConfig(eos_token=EOS)


def _doc_cfg(token_file, **kw):
    return TrainConfig(model=kw.pop("model", "llama-tiny"), micro_batch=1,
                       grad_accum=1, seq_len=64, data_path=token_file,
                       eos_token=EOS, doc_mask=True, **kw)


def test_dense_trainer_passes_bounds_to_the_model(token_file, monkeypatch):
    from trainingjob_operator_amd.models.llama import LlamaModel
    from trainingjob_operator_amd.training import Trainer
    tr = Trainer(_doc_cfg(token_file), device=torch.device("cpu"))
    seen = []
    real = LlamaModel.forward

    def spy(self, tokens, targets=None, doc_bounds=None):
        seen.append((tokens, doc_bounds))
        return real(self, tokens, targets, doc_bounds)
    monkeypatch.setattr(LlamaModel, "forward", spy)
    loss = tr.train_step()
    assert torch.isfinite(loss)
    (tokens, bounds), = seen
    assert bounds is not None
    assert torch.equal(bounds, doc_bounds_from_eos(tokens, EOS))


def test_tp_and_sp_refuse_doc_mask(token_file):
    from trainingjob_operator_amd.training import Trainer
    for kw in (dict(tp_size=2), dict(tp_size=2, sequence_parallel=True)):
        with pytest.raises(ValueError, match="doc_mask"):
            Trainer(_doc_cfg(token_file, **kw), device=torch.device("cpu"))


def test_pp_cp_ep_trainers_refuse_doc_mask(token_file):
    from trainingjob_operator_amd.parallel.cp import CPTrainer
    from trainingjob_operator_amd.parallel.ep import EPTrainer
    from trainingjob_operator_amd.parallel.pp import PPTrainer
    with pytest.raises(ValueError, match="doc_mask"):
        PPTrainer(_doc_cfg(token_file), stage_idx=0, n_stages=1)
    with pytest.raises(ValueError, match="doc_mask"):
        CPTrainer(_doc_cfg(token_file), device="cpu")
    with pytest.raises(ValueError, match="doc_mask"):
        EPTrainer(_doc_cfg(token_file, model="moe-tiny"))


def test_launcher_flags_reach_the_config(token_file):
    """--doc-mask and --eos-token through the launcher's real parser."""
    from trainingjob_operator_amd.launcher.main import build_parser
    ap = build_parser()
    off = ap.parse_args([])
    assert off.doc_mask is False and off.eos_token == -1
    args = ap.parse_args(["--doc-mask", "--eos-token", "5", "--data-path",
                          token_file])
    assert args.doc_mask is True and args.eos_token == 5
    cfg = TrainConfig(data_path=args.data_path, doc_mask=args.doc_mask,
                      eos_token=args.eos_token)
    assert cfg.doc_mask and cfg.eos_token == 5
    with pytest.raises(ValueError):
        a2 = ap.parse_args(["--doc-mask"])
        TrainConfig(data_path=a2.data_path, doc_mask=a2.doc_mask,
                    eos_token=a2.eos_token)


def test_ps_worker_passes_bounds_to_the_model(token_file, monkeypatch):
    """The parameter-server worker runs the dense model: its batches keep
    their layout (three-tuples) instead of failing to unpack."""
    from trainingjob_operator_amd.models.llama import LlamaModel
    from trainingjob_operator_amd.parallel import ps
    w = ps.PSWorker(_doc_cfg(token_file), worker_index=0, n_ps=1,
                    device="cpu")
    w.bounds = []          # no server in this process: nothing to exchange
    seen = []
    real = LlamaModel.forward

    def spy(self, tokens, targets=None, doc_bounds=None):
        seen.append((tokens, doc_bounds))
        return real(self, tokens, targets, doc_bounds)
    monkeypatch.setattr(LlamaModel, "forward", spy)
    loss = w.train_step()
    assert torch.isfinite(loss)
    (tokens, bounds), = seen
    assert torch.equal(bounds, doc_bounds_from_eos(tokens, EOS))
