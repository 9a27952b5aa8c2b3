"""Float64 reference of torchvision's ``mobilenet_v3_large`` for the MobileNetV3-Large classifier tests: a plain ``torch.nn``
restatement of the published torchvision source (torchvision/models/mobilenetv3.py), with torchvision's module and parameter names, so a
``classifiers.MBNetLarge`` state_dict loads into it with ``strict=True``.  Anchor: 4,207,156 parameters with the 4-class head
(the reference's main_image.py)."""
from functools import partial

from torch import nn

from oracle.conv_models import ConvNormAct

# (in, kernel, expanded, out, squeeze-excitation, activation, stride) -- _mobilenet_v3_conf("mobilenet_v3_large")
CONF = [(16, 3, 16, 16, False, "RE", 1), (16, 3, 64, 24, False, "RE", 2), (24, 3, 72, 24, False, "RE", 1),
        (24, 5, 72, 40, True, "RE", 2), (40, 5, 120, 40, True, "RE", 1), (40, 5, 120, 40, True, "RE", 1),
        (40, 3, 240, 80, False, "HS", 2), (80, 3, 200, 80, False, "HS", 1), (80, 3, 184, 80, False, "HS", 1),
        (80, 3, 184, 80, False, "HS", 1), (80, 3, 480, 112, True, "HS", 1), (112, 3, 672, 112, True, "HS", 1),
        (112, 5, 672, 160, True, "HS", 2), (160, 5, 960, 160, True, "HS", 1), (160, 5, 960, 160, True, "HS", 1)]
NORM = partial(nn.BatchNorm2d, eps=0.001, momentum=0.01)


def make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


class SqueezeExcitation(nn.Module):
    """torchvision.ops.SqueezeExcitation(c, sq, scale_activation=nn.Hardsigmoid): ReLU between the two 1x1 convolutions"""

    def __init__(self, c, sq):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(c, sq, 1)
        self.fc2 = nn.Conv2d(sq, c, 1)
        self.activation = nn.ReLU()
        self.scale_activation = nn.Hardsigmoid()

    def forward(self, x):
        return x * self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))


class InvertedResidual(nn.Module):
    def __init__(self, cin, k, cexp, cout, se, act, stride):
        super().__init__()
        A = nn.Hardswish if act == "HS" else nn.ReLU
        self.use_res = stride == 1 and cin == cout
        layers = []
        if cexp != cin:
            layers.append(ConvNormAct(cin, cexp, 1, norm=NORM, act=A))
        layers.append(ConvNormAct(cexp, cexp, k, stride, groups=cexp, norm=NORM, act=A))
        if se:
            layers.append(SqueezeExcitation(cexp, make_divisible(cexp // 4, 8)))
        layers.append(ConvNormAct(cexp, cout, 1, norm=NORM, act=None))
        self.block = nn.Sequential(*layers)

    def forward(self, x):
        y = self.block(x)
        return x + y if self.use_res else y


class MobileNetV3Large(nn.Module):
    def __init__(self, num_classes=4):
        super().__init__()
        layers = [ConvNormAct(3, 16, 3, 2, norm=NORM, act=nn.Hardswish)]
        layers += [InvertedResidual(*row) for row in CONF]
        layers.append(ConvNormAct(160, 960, 1, norm=NORM, act=nn.Hardswish))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Linear(960, 1280), nn.Hardswish(), nn.Dropout(0.2), nn.Linear(1280, num_classes))

    def feature(self, x):
        """the 1280-wide input of the head: hardswish(classifier.0(pooled features))"""
        return self.classifier[1](self.classifier[0](self.avgpool(self.features(x)).flatten(1)))

    def forward(self, x):
        return self.classifier[3](self.classifier[2](self.feature(x)))
