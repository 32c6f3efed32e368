"""The fine-tuning driver's command line against the reference's (tests/golden/finetune_cli.json, recorded from the
reference's parser by tests/golden/make_item_embedding_golden.py): every option with the same name, dest, type,
default and required flag; the driver's additions all carry the --k3m_ prefix."""
import argparse
import json
import os
import sys

from golden_util import HERE, REPO


def _driver_parser():
    sys.path.insert(0, REPO)
    import importlib.util
    spec = importlib.util.spec_from_file_location("k3m_finetune_driver", os.path.join(REPO, "finetune.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_parser()


def _options(parser):
    out = {}
    for a in parser._actions:
        if not a.option_strings or a.dest == "help":
            continue
        flag = isinstance(a, argparse._StoreTrueAction)
        out[a.option_strings[0]] = {"option": a.option_strings[0], "dest": a.dest, "flag": flag,
                                    "type": None if flag or a.type is None else a.type.__name__,
                                    "default": a.default, "required": bool(a.required)}
    return out


def test_parser_matches_the_reference():
    ref = json.load(open(os.path.join(HERE, "golden", "finetune_cli.json")))["options"]
    assert len(ref) >= 40
    got = _options(_driver_parser())
    for o in ref:
        assert o["option"] in got, o["option"]
        assert got[o["option"]] == o, (got[o["option"]], o)
    extra = sorted(set(got) - {o["option"] for o in ref})
    assert extra == ["--k3m_char_tokenizer", "--k3m_max_steps", "--k3m_parity_case", "--k3m_pred_output",
                     "--k3m_synthetic_regions"]


def test_defaults_parse():
    a = _driver_parser().parse_args(["--data_dir", "d", "--output_dir", "o", "--file_name", "f_{}"])
    assert (a.threshold, a.loss_type, a.max_seq_length, a.max_seq_length_pv, a.max_num_pv) == (0.5, "ce", 50, 256, 30)
    assert not (a.do_train or a.do_eval or a.do_pred or a.use_image or a.with_coattention or a.fp16)
    assert a.k3m_pred_output == "reference" and a.k3m_max_steps == 0 and a.k3m_parity_case == ""
