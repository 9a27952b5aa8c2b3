#!/usr/bin/env python
"""Generate tests/golden/classifier_state_dict_layout.json by running the reference's text classifiers.

Run in the build container only (needs the reference checkout, like make_goldens.py):

    python tests/golden/make_classifier_layout.py

``CVPR_code/text_models.py``'s ``DistilBert`` / ``Bert`` / ``Roberta`` are constructed as they are, except that ``from_pretrained``
(network) builds the model from the published configuration of the named checkpoint instead (``from_config``: same modules, random
weights).  torchvision is not installed: placeholder modules satisfy the import statement only.  What is written is key -> shape of
each module's ``state_dict()``; nothing of the reference's source is copied.
"""
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# config.json of the three hub checkpoints, the fields that set parameter shapes (the others are the classes' defaults)
PUBLISHED = {
    "distilbert-base-uncased": {},
    "bert-base-uncased": {},
    "roberta-base": dict(vocab_size=50265, max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1,
                         bos_token_id=0, eos_token_id=2),
}


def main():
    import transformers
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tv.models = tvm
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tvm
    for cls in (transformers.DistilBertModel, transformers.BertModel, transformers.RobertaModel):
        def from_pretrained(klass, name, *a, **kw):
            return klass(klass.config_class(**PUBLISHED[name]))
        cls.from_pretrained = classmethod(from_pretrained)
    sys.path.insert(0, REF)
    import CVPR_code.text_models as tm
    out = {}
    for name, ctor in (("distilbert", tm.DistilBert), ("bert", tm.Bert), ("roberta", tm.Roberta)):
        m = ctor(4, 0.6)
        out[name] = {k: list(v.shape) for k, v in m.state_dict().items()}
        out[name + "|trainable"] = sorted(k for k, p in m.named_parameters() if p.requires_grad)
    with open(os.path.join(HERE, "classifier_state_dict_layout.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print({k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
