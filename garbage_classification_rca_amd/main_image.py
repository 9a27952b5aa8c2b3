"""Image-only training driver: the reference's ``main_image.py`` on the HIP classifiers (classifiers.py).

    python main_image.py --image_model=transformer_B16 --dataset_folder_name=<name> --tl --opt=sgd ...

Data: ``<dataset_folder_name>_Train`` / ``_Val`` under the working directory.  Batch sizes and ``--acc_steps`` come from the reference's
per-model table (main_image.py:264-356); the schedule, checkpoints and accuracy passes are single_modality.train's.  Backbones not built
here print ``Invalid Model`` and exit 1 -- ``b4``, the parser's default, included.
"""
from __future__ import annotations

from .classifiers import IMAGE_FACTORIES
from .single_modality import train

# main_image.py:264-356: model -> (batch size, fine-tuning batch size, forced --acc_steps or None), every model the reference knows
REFERENCE_BATCHES = {
    "b0": (256, 256, None), "b4": (256, 42, None), "b5": (128, 16, 2), "eff_v2_small": (96, 64, None),
    "eff_v2_medium": (128, 24, 12), "eff_v2_large": (96, 12, 6), "res18": (128, 224, None), "res50": (64, 80, None),
    "res152": (64, 38, 2), "mb": (256, 256, None), "convnext": (128, 120, 0), "transformer_B16": (128, 200, None),
    "transformer_L16": (128, 52, 3), "shuffle_net": (128, 52, 3),
}
BATCHES = {k: v for k, v in REFERENCE_BATCHES.items() if k in IMAGE_FACTORIES}


def build_model(name, args, dtype, device):
    return IMAGE_FACTORIES[name](4, args.tl, dtype=dtype, device=device, image_size=args.image_size)


def main(argv=None):
    train("image", argv, build_model, BATCHES)


if __name__ == '__main__':
    main()
