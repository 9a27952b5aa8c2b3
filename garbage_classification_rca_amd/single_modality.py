"""What ``main_image.py`` / ``main_text.py`` and ``calculate_test_accuracy_image.py`` / ``_text.py`` share: the reference's image-only and
text-only drivers (main_image.py / main_text.py) and evaluators on the HIP classifiers (classifiers.py).

The training step, the optimizers and the accuracy passes are the multimodal driver's (training.run_one_epoch /
calculate_set_accuracy, optim.FlatSGD / FlatAdamW, GraphedTrainStep under --hip_graph): a single-modality batch is handed to them with a
placeholder for the missing modality (``_OneModality``), which the classifier engine never reads.
"""
from __future__ import annotations

import math
import os
import sys
import time
from datetime import datetime
from pathlib import Path

import numpy as np
import torch

from .CustomImageTextFolder import CustomImageTextFolder
from .optim import FlatAdamW, FlatSGD
from .options import args_parser
from .training import (calculate_set_accuracy, get_class_weights_from_counts, mode_config_dict, run_one_epoch, stage_images,
                       trim_caption_columns)

_num_classes = 4
TRAIN_DATASET_PATH, VAL_DATASET_PATH = "Train", "Val"
REPORT_PATH = "./test_set_reports"          # calculate_test_accuracy_{image,text}.py: BASE_PATH
CLASS_NAMES = ["Black", "Blue", "Green", "TTR"]


def invalid_model(name, built):
    """an unbuilt backbone: the reference's message, then what this build offers; never a silent substitution"""
    print("Invalid Model: {}".format(name))
    print("Backbones built on the HIP path: {}".format(", ".join(built)))
    sys.exit(1)


def no_image(path):
    """dataset loader of the text-only scripts: the image file is never opened (the reference decodes it through a dummy pipeline
    and ignores it)"""
    return 0


class _OneModality:
    """A DataLoader seen through the multimodal batch layout that training.run_one_epoch / calculate_set_accuracy read: image batches
    get a one-column placeholder caption, caption batches an empty image tensor."""

    def __init__(self, loader, kind):
        self.loader, self.kind = loader, kind

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for data, labels in self.loader:
            n = len(labels)
            if self.kind == "image":
                data["text"] = {"tokens": torch.zeros(n, 1, dtype=torch.int64), "attention_mask": torch.ones(n, 1, dtype=torch.int64)}
            else:
                data["image"]["raw_image"] = torch.zeros(n, 0)
            yield data, labels


class _PairCall:
    """a classifier under the MM_RCA call contract of the accuracy passes (keyword inputs, eval / remove_* flags ignored)"""

    def __init__(self, model):
        self.m, self.engine = model, model.engine

    def __call__(self, _input_ids=None, _attention_mask=None, _images=None, eval=False, remove_text=False, remove_image=False):
        return self.m(_images) if self.m.kind == "image" else self.m(_input_ids, _attention_mask)


def class_weights_of(path):
    ds = CustomImageTextFolder(path, loader=no_image)
    return get_class_weights_from_counts([len(ds.per_class[i]) for i in range(_num_classes)])


def save_model_weights(model, model_name, epoch_num, val_acc, fine_tuning, opt, args, kind):
    """main_image.py:185-210 / main_text.py:213-236: the reference's file names under model_weights/<model>/ (relative to the working
    directory, as in this port); state_dict tensors are copied to the host instead of moving the module"""
    base = os.path.join("model_weights", model_name)
    Path(base).mkdir(parents=True, exist_ok=True)
    if kind == "image":
        if fine_tuning:
            filename = "BEST_model_{}_FT_EPOCH_{}_LR_{}_Reg_{}_Opt_{}_FractionLR_{}_VAL_ACC_{:.5f}_".format(
                model_name, epoch_num + 1, args.lr, args.reg, opt, args.fraction_lr, val_acc)
        else:
            filename = "BEST_model_{}_epoch_{}_LR_{}_Reg_{}_Opt_{}_VAL_ACC_{:.5f}_".format(model_name, epoch_num + 1, args.lr, args.reg, opt, val_acc)
    else:
        if fine_tuning:
            filename = "BEST_model_{}_FT_EPOCH_{}_LR_{}_Reg_{}_FractionLR_{}_OPT_{}_VAL_ACC_{:.5f}_".format(
                model_name, epoch_num + 1, args.lr, args.reg, args.fraction_lr, opt, val_acc)
        else:
            filename = "BEST_model_{}_epoch_{}_LR_{}_Reg_{}_VAL_ACC_{:.5f}_".format(model_name, epoch_num + 1, args.lr, args.reg, val_acc)
    full_path = os.path.join(base, filename + datetime.now().strftime("%Y_%m_%d_%H_%M_%S")) + ".pth"
    print("Saving weights to {}".format(full_path))
    torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, full_path)
    return full_path


def train(kind, argv, build_model, batch_table):
    """main_image.py:233-710 / main_text.py:243-610: two phases (backbone frozen by --tl / by the text constructor for --epochs, then
    everything trainable for --ft_epochs at lr / --fraction_lr), train + val accuracy per epoch, best-val checkpoint,
    ReduceLROnPlateau('max') stepped in the fine-tuning loop only."""
    args = args_parser(argv)
    if args.tl is True:
        print("In Transfer Learning mode!!!")
    if args.dataset_folder_name == "":
        print("Please provide dataset path")
        sys.exit(1)
    name = args.image_model if kind == "image" else args.text_model
    print("{} Model: {}".format("Image" if kind == "image" else "Text", name))
    if name not in batch_table:
        invalid_model(name, list(batch_table))
    if not torch.cuda.is_available():
        print("GPU not available!!!!  The classifier HIP path has no CPU fallback.")
        sys.exit(1)
    if args.seed is not None:
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    _batch_size, _batch_size_FT, acc = batch_table[name]
    if acc is not None:
        args.acc_steps = acc
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}.get(args.dtype, args.dtype)
    global_model = build_model(name, args, dtype, device)
    print("Num total parameters of the model: {}".format(sum(p.numel() for p in global_model.parameters())))
    print("Batch Size: {}".format(_batch_size))
    print("Batch Size FT: {}".format(_batch_size_FT))
    print("Learning Rate: {}".format(args.lr))
    print("Regularization Rate: {}".format(args.reg))
    print("Using class weights: {}".format(args.balance_weights))
    print("Optimizer: {}".format(args.opt))
    print("Grad Acc steps: {}".format(args.acc_steps))
    for flag, default in (("use_synonyms", False), ("prob_aug_text", 0.6)):
        if getattr(args, flag, default) != default:
            print("WARNING: --{} is accepted for CLI compatibility but not implemented on this path (SURVEY.md section 2: out of scope)".format(flag))
    if args.calculate_dataset_stats and kind != "image":
        print("WARNING: --calculate_dataset_stats is accepted for CLI compatibility; the ImageNet mean / std are used, as in main_both.py")

    train_path = "_".join([args.dataset_folder_name, TRAIN_DATASET_PATH])
    val_path = "_".join([args.dataset_folder_name, VAL_DATASET_PATH])
    class_weights = class_weights_of(train_path)
    print("Class weights: {}".format(class_weights))
    image_pipeline, aug_params, collate = None, None, None
    if kind == "image":
        from .main_both import Transforms, decode_only
        WIDTH, HEIGHT = global_model.get_image_size()
        gpu_pre = bool(args.gpu_preprocess)
        norm = {}           # A.Normalize constants for the train and validation pipelines; empty = ImageNet's
        if args.calculate_dataset_stats:
            # main_image.py:425-437: the training set's own statistics at the model's input size, STATS_PIPELINE = stretch resize
            from . import dataset_stats
            print("Calculating Train Dataset statistics...")
            sums, batch_sizes = dataset_stats.compute(train_path, WIDTH, HEIGHT, device, pad=False, seed=args.seed, num_workers=args.num_workers)
            mean_train, std_train = dataset_stats.report(sums, batch_sizes, WIDTH * HEIGHT)
            norm = dict(mean=mean_train, std=std_train)
        if gpu_pre:
            (train_data, collate), (val_data, _) = decode_only(train_path), decode_only(val_path)
            # the reference's TRAIN_PIPELINE / VALIDATION_PIPELINE (main_image.py:409-446) are main_both.py's lists
            from .preprocess import GpuImagePipeline, sample_train_params
            image_pipeline = GpuImagePipeline(HEIGHT, WIDTH, max_batch=max(_batch_size, _batch_size_FT), max_pixels=640 * 480, device=device, **norm)
            aug_rng = np.random.default_rng(None if args.seed is None else int(args.seed) + 7919)
            aug_params = lambda n: sample_train_params(aug_rng, n, args.prob_aug)      # noqa: E731
        else:
            train_data = CustomImageTextFolder(root=train_path, transform=Transforms(WIDTH, HEIGHT, True, args.prob_aug, **norm))
            val_data = CustomImageTextFolder(root=val_path, transform=Transforms(WIDTH, HEIGHT, **norm))
            print("CPU image transforms (--gpu_preprocess=false): of the training augmentations only the flips are applied")
    else:
        WIDTH = HEIGHT = 0
        tok = global_model.get_tokenizer()
        max_len = args.tokens_max_len or global_model.get_max_token_size()
        train_data = CustomImageTextFolder(root=train_path, tokens_max_len=max_len, tokenizer_text=tok, loader=no_image,
                                           extended_desc=args.extended_desc_train)
        val_data = CustomImageTextFolder(root=val_path, tokens_max_len=max_len, tokenizer_text=tok, loader=no_image,
                                         extended_desc=args.extended_desc_val)
    print(train_data.class_to_idx)

    def loader(ds, bs):
        nw = min(args.num_workers, 16)
        ctx = "forkserver" if (image_pipeline is not None and nw > 0) else None
        return _OneModality(torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=True, num_workers=nw, pin_memory=True, collate_fn=collate,
                                                        multiprocessing_context=ctx), kind)

    dl_train, dl_val = loader(train_data, _batch_size), loader(val_data, _batch_size)
    print("Total num of train samples: {}".format(len(train_data)))
    if args.opt == "adamw":
        optimizer = FlatAdamW(global_model, lr=args.lr, weight_decay=args.reg)
    elif args.opt == "sgd":
        optimizer = FlatSGD(global_model, lr=args.lr, weight_decay=args.reg)
    else:
        print("Invalid optimizer!")
        sys.exit(1)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, 'max', factor=0.2 if kind == "image" else 0.4)
    state = dict(max_val=0.0, best_epoch=0)
    graphs = {}
    evaluator = _PairCall(global_model)
    both = mode_config_dict['both']

    def one_phase(n_epochs, dl_tr, dl_v, bs, fine_tuning):
        tag = "Fine Tuning: " if fine_tuning else ""
        for epoch in range(n_epochs):
            global_model.train()
            st = time.time()
            use_graph = args.hip_graph == "on" or (args.hip_graph == "auto" and bs <= 16 and max(WIDTH, 1) * max(HEIGHT, 1) <= 224 * 224)
            # (the reference's fine-tuning loop steps with --acc_steps as well, main_image.py:634 / main_text.py:546)
            _, losses = run_one_epoch(epoch, global_model, dl_tr, len(train_data), device, bs, optimizer, class_weights, args.balance_weights,
                                      args.acc_steps, args.label_smoothing, image_pipeline=image_pipeline, aug_params=aug_params,
                                      hip_graph=(graphs if use_graph else None))
            elapsed = time.time() - st
            print("{}epoch time: {:.1f}".format(tag, elapsed))
            loss_avg = float(np.average([float(l) for l in losses])) if losses else float("nan")
            print("{}avg train loss on epoch {}: {:.3f}".format(tag, epoch, loss_avg))
            global_model.eval()
            train_acc, _ = calculate_set_accuracy(evaluator, dl_tr, len(train_data), device, _batch_size, both, True,
                                                  image_pipeline=image_pipeline, aug_params=aug_params)
            print("{}train set accuracy on epoch {}: {:.3f}".format(tag, epoch, train_acc))
            val_acc, _ = calculate_set_accuracy(evaluator, dl_v, len(val_data), device, _batch_size, both, True, image_pipeline=image_pipeline)
            print("{}Val set accuracy on epoch {}: {:.3f}".format(tag, epoch, val_acc))
            if fine_tuning:
                scheduler.step(val_acc)                # main_image.py:687 / main_text.py:587
            if val_acc > state["max_val"]:
                print("{}best model obtained based on Val Acc. Saving it!".format(tag))
                save_model_weights(global_model, name, epoch, val_acc, fine_tuning, args.opt, args, kind)
                state["max_val"], state["best_epoch"] = val_acc, epoch
            else:
                print("{}not saving model, best Val Acc so far on epoch {}: {:.3f}".format(tag, state["best_epoch"], state["max_val"]))

    one_phase(args.epochs, dl_train, dl_val, _batch_size, False)
    print("Starting Fine tuning!!")
    if args.tl is True:
        for p in global_model.parameters():
            p.requires_grad = True
        for group in optimizer.param_groups:
            group['lr'] = args.lr / args.fraction_lr
        one_phase(args.ft_epochs, loader(train_data, _batch_size_FT), loader(val_data, _batch_size_FT), _batch_size_FT, True)


def calculate_test_accuracy(model, data_loader, len_test_data, device, batch_size, image_pipeline=None):
    """calculate_test_accuracy_{image,text}.py: argmax over the test split -> (accuracy %, text report, report dict, confusion matrix)"""
    from .calculate_test_accuracy_both import confusion_matrix
    correct, all_preds, all_labels = 0, [], []
    evaluator = _PairCall(model)
    n_batches = math.ceil(len_test_data / batch_size)
    with torch.no_grad():
        for batch_idx, (data, labels) in enumerate(data_loader):
            if model.kind == "image":
                out = evaluator(_images=stage_images(data['image']['raw_image'], device, image_pipeline))
            else:
                tok, msk = trim_caption_columns(data['text']['tokens'], data['text']['attention_mask'])
                out = evaluator(_input_ids=tok.to(device), _attention_mask=msk.to(device))
            labels = labels.to(device)
            pred = torch.max(out, 1)[1].view(-1)
            correct += int(torch.sum(torch.eq(pred, labels)).item())
            all_preds += pred.cpu().tolist()
            all_labels += labels.cpu().tolist()
            print("Test batches {}/{} ".format(batch_idx, n_batches))
    acc = 100 * (correct / max(len_test_data, 1))
    cm = confusion_matrix(all_labels, all_preds)
    print(cm)
    try:
        from sklearn.metrics import classification_report
        kw = dict(labels=list(range(_num_classes)), target_names=CLASS_NAMES, zero_division=0)
        report = classification_report(all_labels, all_preds, **kw)
        report_dict = classification_report(all_labels, all_preds, output_dict=True, **kw)
    except Exception:
        report, report_dict = "", {}
    return acc, report, report_dict, cm


def write_report(report_dict, cm, csv_name, png_name, model_name):
    """calculate_test_accuracy_image.py:114-131 / _text.py:114-133: ./test_set_reports/<model>/<csv_name>, the confusion matrix beside it"""
    import pandas as pd
    out = os.path.join(REPORT_PATH, model_name)
    Path(out).mkdir(parents=True, exist_ok=True)
    csv_path = os.path.join(out, csv_name)
    pd.DataFrame.from_dict(report_dict).to_csv(csv_path, index=True)
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        plt.rcParams.update({'font.size': 16})
        fig, ax = plt.subplots(figsize=(10, 5))
        im = ax.imshow(cm, cmap='viridis')
        ax.set_xticks(range(_num_classes)); ax.set_yticks(range(_num_classes))
        ax.set_xticklabels(CLASS_NAMES); ax.set_yticklabels(CLASS_NAMES)
        for i in range(_num_classes):
            for j in range(_num_classes):
                ax.text(j, i, str(int(cm[i, j])), ha="center", va="center", color="w")
        fig.colorbar(im)
        fig.savefig(os.path.join(out, png_name))
        plt.close(fig)
    except Exception as e:      # plotting is optional
        print(f"[mmrca] confusion-matrix image skipped ({type(e).__name__}: {e})")
    print("Report written to {}".format(csv_path))
    return csv_path
