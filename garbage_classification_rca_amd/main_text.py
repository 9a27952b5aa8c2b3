"""Text-only training driver: the reference's ``main_text.py`` on the HIP classifiers (classifiers.py).

    python main_text.py --text_model=distilbert --dataset_folder_name=<name> --tl --opt=sgd ...

Data: ``<dataset_folder_name>_Train`` / ``_Val`` under the working directory; captions only (no image is decoded).  Batch sizes and
``--acc_steps`` come from the reference's per-model table (main_text.py:270-306); the encoder is frozen by the model's constructor and
only ``--tl`` unfreezes it, for the fine-tuning phase.  Backbones not built here print ``Invalid Model`` and exit 1.
"""
from __future__ import annotations

from .classifiers import TEXT_FACTORIES, build_text_classifier
from .single_modality import train

# main_text.py:270-306: model -> (batch size, fine-tuning batch size, forced --acc_steps or None)
REFERENCE_BATCHES = {
    "distilbert": (128, 86, None), "roberta": (128, 42, None), "bert": (128, 26, 3), "bart": (32, 2, 24), "gpt2": (18, 4, 12),
    "mobile_bert": (18, 4, 12),
}
BATCHES = {k: v for k, v in REFERENCE_BATCHES.items() if k in TEXT_FACTORIES}


def build_model(name, args, dtype, device):
    return build_text_classifier(name, 4, args.model_dropout, dtype, device)


def main(argv=None):
    train("text", argv, build_model, BATCHES)


if __name__ == '__main__':
    main()
