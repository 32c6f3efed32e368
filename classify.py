"""Item-classification driver: fine-tunes c_final -> category on labelled single items and predicts the
top-k categories, with finetune.py's option names wherever the meaning is the same.

    python classify.py --data_dir DIR --output_dir OUT --file_name "items_{}" --use_image --with_coattention \
        --do_train --do_eval --do_pred [options]

Records: ``file_name.format("train")`` for training, ``file_name.format("valid")`` for evaluation and prediction, each a
``k3m_amd.loaders.write_records`` directory or a raw product TSV (id, title, image url, KG, category); the category
column is the label.  Files: ``<output_dir>/<config_file>`` is read (BertConfig JSON); ``<output_dir>/
k3m_<model_name>_<layers>l_<heads>h/`` receives ``hyperparamter.txt``, ``labels.json`` (the category of every output
row, built from the training split; evaluation and prediction load it), the per-epoch
``K3M_item_classification-<p>_epoch-<e>.bin`` and the predictions.

* ``--file_state_dict`` seeds the model from any .bin of this project or the reference: a pretraining or an alignment
  file seeds the encoder, its differently shaped ``classifier.*`` entries are left out with a warning;
* ``--label_smoothing E`` and ``--class_weights {none,balanced}`` (N / (C n_c) from the training split) shape the loss;
* ``--eval_topk K``: accuracy@1 and accuracy@K, macro-F1 and the count of left-out (unlabelled) rows are logged;
* ``--k3m_pred_output PATH``: one JSON line per item, ``{"item_id", "pred": top-k categories, "logp"}`` (default
  ``classification_top<k>.jsonl`` in the checkpoint directory);
* ``--fp16`` selects the bf16 encoder with fp32 master weights, as in finetune.py; single GPU only;
* ``--k3m_char_tokenizer``, ``--k3m_synthetic_regions SEED`` (regions for a raw TSV) and ``--k3m_max_steps N`` are the
  build-side options of the other drivers.
"""
import argparse
import logging
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

logging.basicConfig(format="%(asctime)s %(levelname)-4s [%(filename)s:%(lineno)s]  %(message)s",
                    datefmt="%Y/%m/%d %H:%M:%S", level=logging.INFO)
logger = logging.getLogger(__name__)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--data_dir", required=True, type=str, help="directory of the item records")
    p.add_argument("--output_dir", required=True, type=str, help="config file; checkpoints and predictions go below")
    p.add_argument("--file_name", required=True, type=str, help="record name ('{}' -> train / valid)")
    p.add_argument("--model_name", default="bert-base-uncased", type=str)
    p.add_argument("--pretrained_model_path", default=None, type=str, help="directory with vocab.txt")
    p.add_argument("--config_file", default="bert_base_6layer_6conect.json", type=str)
    p.add_argument("--file_state_dict", default=None, type=str, help="seed the model from a .bin")
    p.add_argument("--log_steps", default=1, type=int)
    p.add_argument("--do_train", action="store_true")
    p.add_argument("--do_eval", action="store_true")
    p.add_argument("--do_pred", action="store_true")
    p.add_argument("--use_image", action="store_true")
    p.add_argument("--seed", default=42, type=int)
    p.add_argument("--train_batch_size", default=32, type=int)
    p.add_argument("--eval_batch_size", default=32, type=int)
    p.add_argument("--learning_rate", default=1e-4, type=float)
    p.add_argument("--num_train_epochs", default=6.0, type=float)
    p.add_argument("--start_epoch", default=0, type=float)
    p.add_argument("--if_pre_sampling", default=1, type=int)
    p.add_argument("--with_coattention", action="store_true")
    p.add_argument("--freeze", default=-1, type=int)
    p.add_argument("--warmup_proportion", default=0.1, type=float)
    p.add_argument("--adam_epsilon", default=1e-8, type=float)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--do_lower_case", default=True, type=bool)
    p.add_argument("--max_seq_length", default=50, type=int)
    p.add_argument("--max_seq_length_pv", default=256, type=int)
    p.add_argument("--max_num_pv", default=30, type=int)
    p.add_argument("--max_region_length", default=36, type=int)
    p.add_argument("--dynamic_attention", action="store_true")
    # the classification task's own options
    p.add_argument("--label_smoothing", default=0.0, type=float)
    p.add_argument("--class_weights", default="none", type=str, choices=["none", "balanced"])
    p.add_argument("--eval_topk", default=5, type=int)
    # build-side options
    p.add_argument("--k3m_char_tokenizer", action="store_true")
    p.add_argument("--k3m_synthetic_regions", default=None, type=int)
    p.add_argument("--k3m_max_steps", default=0, type=int)
    p.add_argument("--k3m_pred_output", default="", type=str)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    from k3m_amd import ops
    from k3m_amd.classify import (LABELS_FILE, ItemClassificationTrainer, evaluate, load_encoder, save_model,
                                  write_predictions)
    from k3m_amd.config import BertConfig, classify_config
    from k3m_amd.data import LabelVocab
    from k3m_amd.loaders import CharTokenizer, K3MItemLoader, open_records

    if not (args.do_train or args.do_eval or args.do_pred):
        raise SystemExit("classify.py: nothing to do (--do_train / --do_eval / --do_pred)")
    if not 1 <= args.eval_topk <= ops.TOPK_LOGITS_MAX_K:
        raise SystemExit("--eval_topk %d: between 1 and %d" % (args.eval_topk, ops.TOPK_LOGITS_MAX_K))
    if not torch.cuda.is_available():
        raise SystemExit("classify.py runs the HIP engine; there is no CPU path in this build")
    dev = torch.device("cuda")
    logger.info(f"device: {dev}, n_gpu: 1, 16-bits training: {args.fp16}")
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)

    cfg_path = os.path.join(args.output_dir, args.config_file)
    base = BertConfig.from_json_file(cfg_path)
    model_path = f"k3m_{args.model_name}_{base.num_hidden_layers}l_{base.num_attention_heads}h"
    output_model_path = os.path.join(args.output_dir, model_path)
    os.makedirs(output_model_path, exist_ok=True)
    labels_path = os.path.join(output_model_path, LABELS_FILE)

    rkw = dict(v_feature_size=base.v_feature_size, v_target_size=1601, synthetic_regions=args.k3m_synthetic_regions)
    train_records = valid_records = None
    if args.do_train:
        train_records = open_records(args.data_dir, args.file_name.format("train"), **rkw)
        vocab = LabelVocab.from_records(train_records)
        if len(vocab) < 1:
            raise SystemExit("the training split has no labelled record (empty category column)")
        vocab.save(labels_path)
        logger.info(f"{len(vocab)} categories from the training split -> {labels_path}")
    else:
        if not os.path.exists(labels_path):
            raise SystemExit("%s not found: train first (--do_train writes it)" % labels_path)
        vocab = LabelVocab.load(labels_path)
    if args.do_eval or args.do_pred:
        valid_records = open_records(args.data_dir, args.file_name.format("valid"), **rkw)

    config = classify_config(cfg_path, len(vocab), use_image=args.use_image, with_coattention=args.with_coattention,
                             if_pre_sampling=args.if_pre_sampling, dynamic_attention=args.dynamic_attention,
                             label_smoothing=args.label_smoothing)
    if args.freeze > config.t_biattention_id[0]:   # as finetune.py
        config.fixed_t_layer = config.t_biattention_id[0]
    with open(os.path.join(output_model_path, "hyperparamter.txt"), "w") as f:
        print(args, file=f)
        print("\n", file=f)
        print(config, file=f)

    if args.k3m_char_tokenizer:
        tokenizer = CharTokenizer()
    else:
        from pytorch_transformers.tokenization_bert import BertTokenizer
        tokenizer = BertTokenizer.from_pretrained(args.pretrained_model_path, do_lower_case=args.do_lower_case)
        tokenizer.do_basic_tokenize = False
    lkw = dict(device=dev, seed=args.seed, max_seq_len=args.max_seq_length, max_seq_len_pv=args.max_seq_length_pv,
               max_num_pv=args.max_num_pv, max_region_len=args.max_region_length, v_feature_size=base.v_feature_size,
               v_target_size=config.v_target_size)
    train_loader = valid_loader = None
    if train_records is not None:
        train_loader = K3MItemLoader(train_records, tokenizer, vocab, batch_size=args.train_batch_size, **lkw)
    if valid_records is not None:
        valid_loader = K3MItemLoader(valid_records, tokenizer, vocab, batch_size=args.eval_batch_size, shuffle=False,
                                     **lkw)

    num_dataset = train_loader.num_dataset if train_loader is not None else 0
    total = max(1, int(num_dataset / args.train_batch_size) * int(args.num_train_epochs - args.start_epoch))
    weight = None
    if args.class_weights == "balanced":
        if not any(vocab.counts):
            raise SystemExit("--class_weights balanced needs the class counts of a training split (labels.json has none)")
        weight = torch.from_numpy(vocab.balanced_weights())
    tr = ItemClassificationTrainer(config, dev, lr=args.learning_rate, warmup_steps=args.warmup_proportion * total,
                                   total_steps=total, seed=args.seed, eps=args.adam_epsilon,
                                   dtype="bf16" if args.fp16 else "fp32", class_weight=weight)
    model = tr.model
    if args.file_state_dict:
        missing = load_encoder(model, torch.load(args.file_state_dict, map_location="cpu", weights_only=True))
        logger.info(f"loaded {args.file_state_dict} ({len(missing)} tensors of the model not in the file)")

    ks = tuple(sorted({1, args.eval_topk}))

    def run_eval(tag):
        m, _, _ = evaluate(model, valid_loader, ks=ks)
        line = ", ".join(f"accuracy@{k}={m['accuracy@%d' % k]:.4f}" for k in ks)
        line = f"[{tag}] {line}, macro_f1={m['macro_f1']:.4f}, n={m['n']}, left_out={m['unlabelled']}"
        logger.info(line)
        print(line, flush=True)

    steps_done = 0
    if args.do_train:
        logger.info("***** Running training *****")
        logger.info("  Num examples = %d", num_dataset)
        logger.info("  Batch size = %d", args.train_batch_size)
        logger.info("  Num steps = %d", total)
        for epoch in range(int(args.start_epoch), int(args.num_train_epochs)):
            for step, batch in enumerate(train_loader):
                out = tr.step(batch)
                if (step + 1) % args.log_steps == 0:
                    logger.info(f"[Epoch-{epoch} Step-{step}] loss: {int(float(out['loss']) * 1000) / 1000}")
                steps_done += 1
                if args.k3m_max_steps and steps_done >= args.k3m_max_steps:
                    break
            tr.finish()
            if args.do_eval:
                run_eval(f"Epoch-{epoch}")
            logger.info(f"[Epoch-{epoch}] saving model")
            save_model(model, os.path.join(output_model_path,
                                           f"K3M_item_classification-{args.if_pre_sampling}_epoch-{epoch}.bin"), vocab)
            if args.k3m_max_steps and steps_done >= args.k3m_max_steps:
                break
    elif args.do_eval:
        run_eval("Evaluation")

    if args.do_pred:
        path = args.k3m_pred_output or os.path.join(output_model_path, f"classification_top{args.eval_topk}.jsonl")
        n = write_predictions(model, valid_loader, path, vocab, k=args.eval_topk, seed=args.seed)
        logger.info(f"[Prediction] Finished prediction: {n} items -> {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
