"""VGGLoss -- the forward of reference src/losses/vggloss.py (:59-69) around a caller-supplied feature stack.

The reference builds torchvision's pretrained VGG-19 inside its constructor.  Those weights are not part of this package, so the
stack is an argument: `features` is indexable like torchvision's `vgg19().features` (at least 21 modules).  With features=None the
constructor falls back to torchvision's pretrained network when torchvision can be imported.  The convolutions run in torch."""
import torch

_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)
_SLICES = ((0, 2), (2, 7), (7, 12), (12, 21))


class VGGLoss(torch.nn.Module):
    def __init__(self, features=None):
        super().__init__()
        if features is None:
            try:
                import torchvision
            except ImportError as e:
                raise RuntimeError("diner_amd: VGGLoss() without `features` needs torchvision's pretrained VGG-19; pass the feature "
                                   "stack (a torchvision-style vgg19().features with its weights loaded) instead") from e
            features = torchvision.models.vgg19(pretrained=True).features
        if len(features) < _SLICES[-1][1]:
            raise ValueError(f"diner_amd: VGGLoss needs a feature stack of at least {_SLICES[-1][1]} modules, got {len(features)}")
        self.slices = torch.nn.ModuleList(torch.nn.Sequential(*[features[i] for i in range(a, b)]) for a, b in _SLICES)
        for p in self.parameters():
            p.requires_grad = False
        self.l1_loss = torch.nn.L1Loss()
        self.weights = [1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0]

    def _normalize(self, x):
        mean = torch.as_tensor(_MEAN, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        std = torch.as_tensor(_STD, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        return (x - mean) / std

    def forward(self, x, y):
        x, y = self._normalize(x), self._normalize(y)
        loss = 0
        for w, sl in zip(self.weights, self.slices):
            x, y = sl(x), sl(y)
            loss = loss + w * self.l1_loss(x, y.detach())
        return loss
