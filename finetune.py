"""Item-alignment driver with the command line of the reference's ``finetune.py`` (argparse surface :1223-1288,
config mutations :1309-1325, training loop :843-1113, prediction :1116-1212), running the MI355X model:
``k3m_amd.finetune.ItemAlignmentTrainer`` for ``--do_train``, ``evaluate(forward_only=True)`` for ``--do_eval`` and
``write_predictions`` for ``--do_pred`` (item-embedding inference).

    python finetune.py --data_dir DIR --output_dir OUT --file_name "pairs_{}" --use_image --with_coattention \
        --do_train --do_eval --do_pred [reference options]

Same files as the reference: ``<output_dir>/<config_file>`` (BertConfig JSON); ``<output_dir>/
k3m_<model_name>_<layers>l_<heads>h/`` receives ``hyperparamter.txt``, the per-epoch
``K3M_item_alignment-<p>_epoch-<e>.bin`` and ``deepAI_result_threshold=<t>.jsonl``.  Records:
``file_name.format("train")`` for training, ``file_name.format("valid")`` for evaluation and prediction (:721, :821,
:837), each a ``k3m_amd.loaders.write_pair_records`` directory (the tensorpack LMDB container is not read).

Differences, each stated:
* single GPU only (the reference spawns one worker per GPU, :1327-1329);
* ``--fp16`` selects the bf16 encoder with fp32 master weights instead of apex amp; ``--loss_scale`` is accepted and
  unused;
* evaluation concatenates the batches (the reference's ``np.concatenate(model_probs, probs)`` fails from the second
  batch on); the hard gate's draw in evaluation and prediction is seeded by the batch index, so a run is reproducible;
* build-side options, all prefixed ``--k3m_``: ``--k3m_char_tokenizer`` (no vocab.txt offline),
  ``--k3m_synthetic_regions SEED`` (accepted for symmetry with train.py; pair records carry their regions),
  ``--k3m_max_steps N``, ``--k3m_pred_output {reference,embedding}`` (``embedding``: c_final of both items for every
  loss type) and the parity harness ``--k3m_parity_case NPZ``: a ``golden_ft_*`` fixture's pair, weights and gumbel
  noise are fed in place of the loaders (tests/test_gpu_finetune_driver.py);
* ``--do_retrieve`` (the reference has no retrieval step): both items of every ``valid`` pair are embedded,
  the item-2 side is indexed and searched with the item-1 side (``k3m_amd.retrieve``, cosine), one JSON line per pair
  ``{"src_item_id", "tgt_item_ids", "scores"}`` with ``--k3m_topk`` (default 10) ids goes to
  ``--k3m_retrieve_output`` (default ``retrieval_top<k>.jsonl`` beside the predictions) and Rank@1/5/10 over the
  pairs with label 1 is logged.
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
    """The reference's options (finetune.py:1223-1288), same names, types and defaults, then the --k3m_ ones."""
    p = argparse.ArgumentParser()
    p.add_argument("--data_dir", required=True, type=str, help="directory of the pair records")
    p.add_argument("--output_dir", required=True, type=str, help="config file; checkpoints and predictions go below")
    p.add_argument("--file_name", required=True, type=str, help="record name ('{}' -> train / valid)")
    p.add_argument("--model_name", default="bert-base-uncased", type=str)
    p.add_argument("--pretrained_model_path", default=None, type=str, help="directory with vocab.txt")
    p.add_argument("--config_file", default="bert_base_6layer_6conect.json", type=str)
    p.add_argument("--file_checkpoint", default=None, type=str, help="resume from a .tar (accepted, unused)")
    p.add_argument("--file_state_dict", default=None, type=str, help="load model weights from a .bin")
    p.add_argument("--log_steps", default=1, type=int)
    p.add_argument("--cache", default=5000, type=int)
    p.add_argument("--do_train", action="store_true")
    p.add_argument("--do_eval", action="store_true")
    p.add_argument("--do_pred", action="store_true")
    p.add_argument("--use_image", action="store_true")
    p.add_argument("--seed", default=42, type=int)
    p.add_argument("--no_cuda", action="store_true")
    p.add_argument("--train_batch_size", default=32, type=int)
    p.add_argument("--eval_batch_size", default=32, type=int)
    p.add_argument("--learning_rate", default=1e-4, type=float)
    p.add_argument("--num_train_epochs", default=6.0, type=float)
    p.add_argument("--start_epoch", default=0, type=float)
    p.add_argument("--num_workers", default=8, type=int)
    p.add_argument("--if_pre_sampling", default=1, type=int)
    p.add_argument("--with_coattention", action="store_true")
    p.add_argument("--freeze", default=-1, type=int)
    p.add_argument("--threshold", default=0.5, type=float)
    p.add_argument("--warmup_proportion", default=0.1, type=float)
    p.add_argument("--gradient_accumulation_steps", default=1, type=int)
    p.add_argument("--adam_epsilon", default=1e-8, type=float)
    p.add_argument("--loss_img_weight", default=1, type=float)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--loss_type", default="ce", type=str)
    p.add_argument("--loss_scale", default=0, type=float)
    p.add_argument("--do_lower_case", default=True, type=bool)
    p.add_argument("--max_seq_length", default=50, type=int)
    p.add_argument("--max_seq_length_pv", default=256, type=int)
    p.add_argument("--max_num_pv", default=30, type=int)
    p.add_argument("--max_region_length", default=36, type=int)
    p.add_argument("--dynamic_attention", action="store_true")
    p.add_argument("--visual_target", default=0, type=int)
    p.add_argument("--num_negative_image", default=255, type=int)
    # build-side options (module docstring)
    p.add_argument("--k3m_char_tokenizer", action="store_true")
    p.add_argument("--k3m_synthetic_regions", default=None, type=int)
    p.add_argument("--k3m_max_steps", default=0, type=int)
    p.add_argument("--k3m_parity_case", default="", type=str)
    p.add_argument("--k3m_pred_output", default="reference", type=str, choices=["reference", "embedding"])
    return p


def build_retrieve_parser():
    """The retrieval step's options.  A parser of their own: build_parser() stays the reference's
    surface plus the build-side options, which tests/test_finetune_cli.py pins option by option."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--do_retrieve", action="store_true")
    p.add_argument("--k3m_topk", default=10, type=int)
    p.add_argument("--k3m_retrieve_output", default="", type=str)
    return p


def parse_args(argv=None):
    """The driver's whole command line -> (args of build_parser(), the retrieval options): the retrieval options
    are taken out first, build_parser() reads the rest (and rejects what neither knows).  Two namespaces, so that
    what the driver records of ``args`` (hyperparamter.txt) is what it was."""
    rargs, rest = build_retrieve_parser().parse_known_args(argv)
    return build_parser().parse_args(rest), rargs


def _parity_inputs(path, dev):
    """(pair dict with item ids, noise pair, fixture) of a golden_ft_* case (tests/golden/make_finetune_golden.py)."""
    d = np.load(path, allow_pickle=False)
    g = {k: d[k] for k in d.files}
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g["out/" + k]))  # noqa: E731
    image = "out/coll_image_feat_1" in g
    pair = {"labels": t("labels")}
    for k in (1, 2):
        for a, b in (("input_ids", "input_ids"), ("token_type_ids", "segment_ids"), ("attention_mask", "input_mask"),
                     ("input_ids_pv", "input_ids_pv"), ("token_type_ids_pv", "segment_ids_pv"),
                     ("attention_mask_pv", "input_mask_pv"), ("index_p", "index_p"), ("index_v", "index_v")):
            pair["%s_%d" % (a, k)] = t("%s_%d" % (b, k))
        if image:
            pair["image_feat_%d" % k] = t("coll_image_feat_%d" % k).float()
            pair["image_loc_%d" % k] = t("coll_image_loc_%d" % k)
            pair["image_attention_mask_%d" % k] = t("coll_image_mask_%d" % k)
    pair = {k: v.to(dev) for k, v in pair.items()}
    B, T = pair["input_ids_1"].shape
    P = pair["input_ids_pv_1"].shape[1]
    scale = float(g["noise_scale"]) if "noise_scale" in g else 1.0
    noise = []
    for s in (int(g["noise_seed"]), int(g["noise_seed"]) + 1):
        rng = np.random.default_rng(s)
        shapes = ([("v", (B, pair["image_feat_1"].shape[1], 3, 1024)), ("t", (B, T, 3, 768)), ("pv", (B, P, 3, 768))]
                  if image else [("t", (B, T, 2, 768)), ("pv", (B, P, 2, 768))])
        noise.append({k: torch.from_numpy((scale * -np.log(rng.standard_exponential(sh))).astype(np.float32)).to(dev)
                      for k, sh in shapes})
    pair["item_ids_1"] = ["src-%d" % i for i in range(B)]
    pair["item_ids_2"] = ["tgt-%d" % i for i in range(B)]
    return pair, tuple(noise), g


def main(argv=None):
    args, rargs = parse_args(argv)
    from k3m_amd import checkpoint as C
    from k3m_amd.config import finetune_config
    from k3m_amd.finetune import ItemAlignmentTrainer, evaluate, save_model, write_predictions

    if args.no_cuda or not torch.cuda.is_available():
        raise SystemExit("finetune.py runs the HIP engine; there is no CPU path in this build")
    dev = torch.device("cuda")
    logger.info(f"device: {dev}, n_gpu: 1, 16-bits training: {args.fp16}")
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)

    cfg_path = os.path.join(args.output_dir, args.config_file)
    parity = _parity_inputs(args.k3m_parity_case, dev) if args.k3m_parity_case else None
    kw = dict(loss_type=args.loss_type, use_image=args.use_image, with_coattention=args.with_coattention,
              if_pre_sampling=args.if_pre_sampling, visual_target=args.visual_target,
              dynamic_attention=args.dynamic_attention, num_negative_image=args.num_negative_image)
    if parity is not None:   # the fixture's model
        g = parity[2]
        kw.update(loss_type=str(g["loss_type"]), if_pre_sampling=int(g["mode"]), use_image="image_feat_1" in parity[0],
                  with_coattention=bool(int(g["with_coattention"])) if "with_coattention" in g else True,
                  dynamic_attention=bool(int(g["dynamic_attention"])) if "dynamic_attention" in g else False)
    config = finetune_config(cfg_path, **kw)
    if args.freeze > config.t_biattention_id[0]:   # :1318-1319
        config.fixed_t_layer = config.t_biattention_id[0]
    model_path = f"k3m_{args.model_name}_{config.num_hidden_layers}l_{config.num_attention_heads}h"
    output_model_path = os.path.join(args.output_dir, model_path)
    os.makedirs(output_model_path, exist_ok=True)
    with open(os.path.join(output_model_path, "hyperparamter.txt"), "w") as f:
        print(args, file=f)
        print("\n", file=f)
        print(config, file=f)

    train_loader = valid_loader = None
    if parity is None:
        if args.k3m_char_tokenizer:
            from k3m_amd.loaders import CharTokenizer
            tokenizer = CharTokenizer()
        else:
            from pytorch_transformers.tokenization_bert import BertTokenizer
            tokenizer = BertTokenizer.from_pretrained(args.pretrained_model_path, do_lower_case=args.do_lower_case)
            tokenizer.do_basic_tokenize = False
        from vilbert_k3m.datasets import K3MDataLoader
        lkw = dict(max_seq_len=args.max_seq_length, max_seq_len_pv=args.max_seq_length_pv, max_num_pv=args.max_num_pv,
                   max_region_len=args.max_region_length, v_target_size=config.v_target_size,
                   visual_target=args.visual_target, num_workers=args.num_workers, device=dev, seed=args.seed)
        if args.do_train:
            train_loader = K3MDataLoader(args.data_dir, args.file_name.format("train"), tokenizer,
                                         batch_size=args.train_batch_size, **lkw)
        if args.do_eval or args.do_pred or rargs.do_retrieve:
            valid_loader = K3MDataLoader(args.data_dir, args.file_name.format("valid"), tokenizer,
                                         batch_size=args.eval_batch_size, shuffle=False, **lkw)

    def train_batches():
        return [parity[0]] * max(1, args.k3m_max_steps) if parity is not None else train_loader

    def valid_batches():
        return [parity[0]] if parity is not None else valid_loader

    num_dataset = train_loader.num_dataset if train_loader is not None else 0
    total = int(num_dataset / args.train_batch_size / args.gradient_accumulation_steps) * \
        int(args.num_train_epochs - args.start_epoch)   # :790-793
    total = max(total, 1)
    tr = ItemAlignmentTrainer(config, dev, lr=args.learning_rate, warmup_steps=args.warmup_proportion * total,
                              total_steps=total, seed=args.seed, eps=args.adam_epsilon,
                              dtype="bf16" if args.fp16 else "fp32")
    model, fp = tr.model, tr.engine.fp
    if parity is not None and "weight_seed" in parity[2]:
        from k3m_amd.weights import param_values
        g = parity[2]
        std = {"std": float(g["weight_std"])} if "weight_std" in g else {}
        fp.load(param_values(config, int(g["weight_seed"]), **std))
    if args.file_state_dict:
        C.load_model_state_dict(fp, torch.load(args.file_state_dict, map_location="cpu", weights_only=True),
                                strict=False)
        logger.info("Successfully loaded model state dict ...")

    def run_eval(tag):
        metrics, _, _ = evaluate(model, valid_batches(), forward_only=True)
        for m in metrics:
            logger.info(f"[{tag}] threshold={m['threshold']}, precision={m['precision']}, recall={m['recall']}, "
                        f"f1={m['f1']}")
            print(f"[{tag}] threshold={m['threshold']:.1f}, precision={m['precision']}, recall={m['recall']}, "
                  f"f1={m['f1']}", flush=True)

    steps_done = 0
    if args.do_train:
        logger.info("***** Running training *****")
        logger.info("  Num examples = %d", num_dataset)
        logger.info("  Batch size = %d", args.train_batch_size)
        logger.info("  Num steps = %d", total)
        for epoch in range(int(args.start_epoch), int(args.num_train_epochs)):
            for step, pair in enumerate(train_batches()):
                out = tr.step(pair, noise=parity[1] if parity is not None else None)
                if (step + 1) % args.log_steps == 0:
                    logger.info(f"[Epoch-{epoch} Step-{step}] loss: {int(float(out['loss']) * 1000) / 1000}")
                steps_done += 1
                if args.k3m_max_steps and steps_done >= args.k3m_max_steps:
                    break
            if args.do_eval:
                run_eval(f"Epoch-{epoch}")
            logger.info(f"[Epoch-{epoch}] saving model")
            save_model(model, os.path.join(output_model_path,
                                           f"K3M_item_alignment-{args.if_pre_sampling}_epoch-{epoch}.bin"))
            if args.k3m_max_steps and steps_done >= args.k3m_max_steps:
                break
    elif args.do_eval:
        run_eval("Evaluation")

    if args.do_pred:
        path = os.path.join(output_model_path, f"deepAI_result_threshold={args.threshold}.jsonl")
        n = write_predictions(model, valid_batches(), path, args.threshold, output=args.k3m_pred_output,
                              noise=[parity[1]] if parity is not None else None, seed=args.seed)
        logger.info(f"[Prediction] Finished prediction: {n} pairs -> {path}")

    if rargs.do_retrieve:
        from k3m_amd.retrieve import retrieve_pairs
        path = rargs.k3m_retrieve_output or os.path.join(output_model_path, f"retrieval_top{rargs.k3m_topk}.jsonl")
        n, ranks = retrieve_pairs(model, valid_batches(), path, k=rargs.k3m_topk,
                                  noise=[parity[1]] if parity is not None else None, seed=args.seed)
        logger.info(f"[Retrieval] {n} queries -> {path}")
        line = ", ".join(f"Rank@{k.split('@')[1]}={v:.4f}" for k, v in ranks.items())
        logger.info(f"[Retrieval] {line}")
        print(f"[Retrieval] {line}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
