"""The host side of item classification, no GPU: the config, the parameter inventory, the label
vocabulary, the metrics against sklearn, the driver's parser and load_encoder's filter."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

from golden_util import CFG_PATH, REPO


def test_classify_config_validation():
    from k3m_amd.config import classify_config, finetune_config
    cfg = classify_config(CFG_PATH, 7, label_smoothing=0.1, if_pre_sampling=2, fixed_t_layer=3)
    assert (cfg.task, cfg.num_labels, cfg.label_smoothing) == ("item_classification", 7, 0.1)
    ft = finetune_config(CFG_PATH, if_pre_sampling=2, fixed_t_layer=3)
    skip = ("task", "num_labels", "label_smoothing")
    assert {k: v for k, v in cfg.to_dict().items() if k not in skip} == \
        {k: v for k, v in ft.to_dict().items() if k not in skip}
    assert classify_config(CFG_PATH, 1).label_smoothing == 0.0
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            classify_config(CFG_PATH, bad)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            classify_config(CFG_PATH, 3, label_smoothing=bad)


@pytest.mark.parametrize("kw", [{}, {"use_image": False}, {"with_coattention": False}, {"if_pre_sampling": 3}])
def test_spec_is_the_alignment_spec_with_a_single_item_head(kw):
    from k3m_amd.config import classify_config, finetune_config
    from k3m_amd.params import frozen_names, is_no_decay, item_alignment_spec, param_spec
    C = 11
    cfg = classify_config(CFG_PATH, C, **kw)
    ft = finetune_config(CFG_PATH, loss_type="ce", **kw)
    spec, ref = param_spec(cfg), item_alignment_spec(ft)
    assert [n for n, _ in spec] == [n for n, _ in ref]
    H = cfg.hidden_size
    want = {"classifier.dense.weight": (H, H), "classifier.dense.bias": (H,), "classifier.out_proj.weight": (C, H),
            "classifier.out_proj.bias": (C,)}
    for (n, s), (_, r) in zip(spec, ref):
        assert tuple(s) == tuple(want.get(n, r)), n
    assert frozen_names(cfg) == frozen_names(ft)
    assert not any(n in frozen_names(cfg) for n in want)
    assert is_no_decay("classifier.out_proj.bias") and not is_no_decay("classifier.out_proj.weight")


def _records(cates):
    return [("id%d" % i, "title", "p:v;", c, 1.0, 1.0, 0, None, None, None) for i, c in enumerate(cates)]


def test_label_vocab(tmp_path):
    from k3m_amd.data import LabelVocab
    v = LabelVocab.from_records(_records(["shoes", "bags", "", "shoes", "hats", "shoes", ""]))
    assert v.names == ["bags", "hats", "shoes"] and v.counts == [1, 1, 3] and len(v) == 3
    assert [v.encode(c) for c in ("bags", "hats", "shoes", "", "socks")] == [0, 1, 2, -1, -1]
    w = v.balanced_weights()
    assert w.dtype == np.float32
    np.testing.assert_allclose(w, [5 / 3.0, 5 / 3.0, 5 / 9.0], rtol=1e-6)
    path = str(tmp_path / "labels.json")
    v.save(path)
    u = LabelVocab.load(path)
    assert (u.names, u.counts) == (v.names, v.counts) and u.encode("hats") == 1
    with pytest.raises(ValueError):
        LabelVocab(["a", "a"])
    with pytest.raises(ValueError):
        LabelVocab(["a", "b"]).balanced_weights()   # no counts


def test_classification_metrics_match_sklearn():
    from sklearn.metrics import accuracy_score, f1_score
    from k3m_amd.classify import classification_metrics
    #                  row: 0  1  2   3  4  5   6  7
    labels = np.array([0, 1, -1, 2, 2, 3, -1, 0])          # class 3 is never predicted, class 4 never a label
    ids = np.array([[0, 1], [2, 1], [1, 0], [2, 0], [0, 1], [4, 0], [3, 3], [1, 2]])
    m = classification_metrics(ids, labels, ks=(1, 2))
    keep = labels != -1
    y, p = labels[keep], ids[keep, 0]
    assert m["n"] == 6 and m["unlabelled"] == 2
    assert m["accuracy@1"] == pytest.approx(accuracy_score(y, p))
    assert m["accuracy@2"] == pytest.approx(3 / 6.0)
    assert m["macro_f1"] == pytest.approx(f1_score(y, p, average="macro", zero_division=0))
    assert m["support"] == {0: 2, 1: 1, 2: 2, 3: 1}
    t = classification_metrics(torch.from_numpy(ids), torch.from_numpy(labels), ks=(1,))
    assert t["accuracy@1"] == m["accuracy@1"] and "accuracy@2" not in t
    e = classification_metrics(np.zeros((2, 1), np.int64), np.array([-1, -1]), ks=(1,))
    assert (e["n"], e["unlabelled"], e["accuracy@1"], e["macro_f1"], e["support"]) == (0, 2, 0.0, 0.0, {})
    with pytest.raises(ValueError):
        classification_metrics(ids, labels, ks=(3,))


def _driver():
    spec = importlib.util.spec_from_file_location("k3m_classify_driver", os.path.join(REPO, "classify.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_parser_defaults():
    p = _driver().build_parser()
    a = p.parse_args(["--data_dir", "d", "--output_dir", "o", "--file_name", "f_{}"])
    assert (a.label_smoothing, a.class_weights, a.eval_topk) == (0.0, "none", 5)
    assert (a.max_seq_length, a.max_seq_length_pv, a.max_num_pv, a.max_region_length) == (50, 256, 30, 36)
    assert (a.train_batch_size, a.eval_batch_size, a.learning_rate, a.num_train_epochs) == (32, 32, 1e-4, 6.0)
    assert (a.if_pre_sampling, a.freeze, a.warmup_proportion, a.file_state_dict) == (1, -1, 0.1, None)
    assert not (a.do_train or a.do_eval or a.do_pred or a.use_image or a.with_coattention or a.fp16)
    assert (a.k3m_char_tokenizer, a.k3m_synthetic_regions, a.k3m_max_steps, a.k3m_pred_output) == (False, None, 0, "")
    with pytest.raises(SystemExit):
        p.parse_args(["--data_dir", "d", "--output_dir", "o", "--file_name", "f", "--class_weights", "sqrt"])


class _FakeFP(object):
    """The part of FlatParams that load_model_state_dict touches, on the host."""

    def __init__(self, cfg):
        from k3m_amd.params import param_spec
        self.spec = param_spec(cfg)
        self.shapes = dict(self.spec)
        self.p = {n: torch.zeros(s) for n, s in self.spec}
        self.shadow_fresh = True


class _FakeModel(object):
    def __init__(self, cfg):
        self.C = cfg.num_labels
        self.engine = type("E", (), {})()
        self.engine.fp = _FakeFP(cfg)


def _small(cfg):
    cfg.vocab_size, cfg.max_position_embeddings, cfg.v_feature_size = 32, 16, 8   # keeps the host tensors small
    cfg.hidden_size = cfg.v_hidden_size = cfg.bi_hidden_size = 16
    cfg.intermediate_size = cfg.v_intermediate_size = 32
    return cfg


def test_load_encoder_leaves_out_a_mismatched_head():
    from k3m_amd.classify import load_encoder
    from k3m_amd.config import classify_config, finetune_config
    from k3m_amd.params import param_spec
    model = _FakeModel(_small(classify_config(CFG_PATH, 4, with_coattention=False)))
    ft = _small(finetune_config(CFG_PATH, loss_type="ce", with_coattention=False))   # an alignment .bin: a pair head
    sd = {"module." + n: torch.full(s, 2.0) for n, s in param_spec(ft)}
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        missing = load_encoder(model, sd)
    text = " ".join(str(w.message) for w in rec)
    for n in ("classifier.out_proj.weight", "classifier.out_proj.bias", "classifier.dense.weight"):
        assert n in text and n in missing, n
    assert "classifier.dense.bias" not in text        # same shape: loaded
    p = model.engine.fp.p
    assert float(p["classifier.out_proj.weight"].abs().max()) == 0.0
    assert float(p["classifier.dense.weight"].abs().max()) == 0.0
    assert bool((p["struc_w1.weight"] == 2.0).all()) and bool((p["classifier.dense.bias"] == 2.0).all())
    assert bool((p["encoder.layer.5.output.dense.weight"] == 2.0).all())
    # a file of this model: nothing left out, nothing missing, no warning
    own = {n: torch.full(s, 3.0) for n, s in model.engine.fp.spec}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert load_encoder(model, own) == []
    assert bool((p["classifier.out_proj.weight"] == 3.0).all())


def test_model_refuses_another_task():
    from k3m_amd.classify import K3MForItemClassification
    from k3m_amd.config import finetune_config
    with pytest.raises(ValueError, match="classify_config"):
        K3MForItemClassification(finetune_config(CFG_PATH))
