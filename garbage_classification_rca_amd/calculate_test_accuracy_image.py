"""Test-split evaluator of the image-only classifiers: the reference's ``calculate_test_accuracy_image.py`` on the HIP path.

    python calculate_test_accuracy_image.py --image_model=transformer_B16 --model_path=<checkpoint.pth> --dataset_folder_name=<Test folder>

Per-model batch sizes of the reference (:152-212), its validation pipeline (pad to the aspect ratio, resize, ImageNet normalisation),
no shuffling, the report CSV ``./test_set_reports/<model>/image_model_<model>_report_test_set_acc_<acc>.csv`` (:114-131) and the
confusion-matrix image beside it.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from .CustomImageTextFolder import CustomImageTextFolder
from .classifiers import IMAGE_FACTORIES
from .options import args_parser
from .single_modality import calculate_test_accuracy, invalid_model, write_report

BATCHES = {"transformer_B16": 128, "transformer_L16": 128, "eff_v2_medium": 32, "eff_v2_large": 8, "shuffle_net": 128, "mb": 256}


def main(argv=None):
    args = args_parser(argv)
    if args.model_path == "":
        print("Please provide test model path")
        sys.exit(0)
    if args.image_model not in BATCHES:
        invalid_model(args.image_model, list(BATCHES))
    if not torch.cuda.is_available():
        print("GPU not available!!!!  The classifier HIP path has no CPU fallback.")
        sys.exit(1)
    device = torch.device("cuda:0")
    torch.manual_seed(42)
    np.random.seed(42)
    _batch_size = BATCHES[args.image_model]
    print("Image Model: {}".format(args.image_model))
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}.get(args.dtype, args.dtype)
    model = IMAGE_FACTORIES[args.image_model](4, args.tl, dtype=dtype, device=device, image_size=args.image_size)
    model.load_state_dict(torch.load(args.model_path, map_location="cpu"))
    model.eval()
    WIDTH, HEIGHT = model.get_image_size()
    from .main_both import Transforms, decode_only
    gpu_pre = bool(args.gpu_preprocess)
    test_data, collate = decode_only(args.dataset_folder_name) if gpu_pre else \
        (CustomImageTextFolder(root=args.dataset_folder_name, transform=Transforms(WIDTH, HEIGHT)), None)
    print("Num of test images: {}".format(len(test_data)))
    pipeline = None
    if gpu_pre:
        from .preprocess import GpuImagePipeline
        pipeline = GpuImagePipeline(HEIGHT, WIDTH, max_batch=_batch_size, max_pixels=640 * 480, device=device)
    nw = min(8, args.num_workers)
    loader = torch.utils.data.DataLoader(test_data, batch_size=_batch_size, shuffle=False, num_workers=nw, pin_memory=True,
                                         collate_fn=collate,
                                         multiprocessing_context="forkserver" if (gpu_pre and nw > 0) else None)
    acc, report, report_dict, cm = calculate_test_accuracy(model, loader, len(test_data), device, _batch_size, pipeline)
    write_report(report_dict, cm, "image_model_{}_report_test_set_acc_{:.2f}.csv".format(args.image_model, acc),
                 "conf_matrix_image_model_{}_test_set_acc_{:.2f}.png".format(args.image_model, acc), args.image_model)
    print(test_data.class_to_idx)
    print("Test accuracy: {:.2f} %".format(acc))
    print("Test Report:")
    print(report)


if __name__ == '__main__':
    main()
