"""Test-split evaluator of the text-only classifiers: the reference's ``calculate_test_accuracy_text.py`` on the HIP path.

    python calculate_test_accuracy_text.py --text_model=distilbert --model_path=<checkpoint.pth> --dataset_folder_name=<Test folder>

Batch 128 (:155-166), seed 42, captions only (no image is decoded), ``--balance_weights`` read from the checkpoint name as the reference
does, the report CSV ``./test_set_reports/<model>/text_model_<model>_report_test_set_acc_<acc>.csv`` (:114-133) and the confusion-matrix
image beside it.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from .CustomImageTextFolder import CustomImageTextFolder
from .classifiers import build_text_classifier
from .options import args_parser
from .single_modality import calculate_test_accuracy, invalid_model, no_image, write_report

BATCHES = {"distilbert": 128, "roberta": 128, "bert": 128, "mobile_bert": 18}     # (:155-177)


def main(argv=None):
    args = args_parser(argv)
    if args.model_path == "":
        print("Please provide test model path")
        sys.exit(0)
    if args.text_model not in BATCHES:
        invalid_model(args.text_model, list(BATCHES))
    if not torch.cuda.is_available():
        print("GPU not available!!!!  The classifier HIP path has no CPU fallback.")
        sys.exit(1)
    torch.manual_seed(42)
    np.random.seed(42)
    device = torch.device("cuda:0")
    _batch_size = BATCHES[args.text_model]
    print("Text Model: {}".format(args.text_model))
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}.get(args.dtype, args.dtype)
    model = build_text_classifier(args.text_model, 4, args.model_dropout, dtype, device)
    model.load_state_dict(torch.load(args.model_path, map_location="cpu"))
    model.eval()
    max_len = args.tokens_max_len or model.get_max_token_size()
    test_data = CustomImageTextFolder(root=args.dataset_folder_name, tokens_max_len=max_len, tokenizer_text=model.get_tokenizer(), loader=no_image)
    print("Num of test texts: {}".format(len(test_data)))
    loader = torch.utils.data.DataLoader(test_data, batch_size=_batch_size, shuffle=True, num_workers=min(8, args.num_workers), pin_memory=True)
    if "true" in args.model_path or "True" in args.model_path:
        args.balance_weights = True
    if "false" in args.model_path or "False" in args.model_path:
        args.balance_weights = False
    acc, report, report_dict, cm = calculate_test_accuracy(model, loader, len(test_data), device, _batch_size)
    write_report(report_dict, cm, "text_model_{}_report_test_set_acc_{:.2f}.csv".format(args.text_model, acc),
                 "conf_matrix_text_model_{}_class_weights_{}_test_set_acc_{:.2f}.png".format(args.text_model, args.balance_weights, acc),
                 args.text_model)
    print(test_data.class_to_idx)
    print("Test accuracy: {:.2f} %".format(acc))
    print("Test Report:")
    print(report)


if __name__ == '__main__':
    main()
