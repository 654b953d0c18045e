"""Drop-in boundary of /root/reference/loss.py: get_loss (:14-43), get_loss_aux (:71-88), ImageBasedCrossEntropyLoss2d (:120-163) and CrossEntropyLoss2d
(:167-180), without the reference's `datasets` / `config` imports.

    from pinthememory_amd.loss import get_loss, get_loss_aux

Inside the networks (network.deepv3plus.segmentation_loss) these criteria never see materialised logits: the fused up-sample + cross-entropy kernels take the
class weights (ops.upsample_wce), and the image-based criterion's weight rows come from the labels on the device (kernels.label_class_weights) -- the reference
computes them with numpy on the host every step (`targets.data.cpu().numpy()`, np.histogram(normed=True), which current numpy no longer accepts), a sync that
cannot be captured into a graph. Called directly on materialised logits (validation code does that) the classes compute the same loss from torch ops.
Relaxed-border labels (`--jointwtborder`, ImgWtLossSoftNLL) are out of scope."""
import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

IGNORE_LABEL = 255      # datasets.ignore_label (/root/reference/datasets/__init__.py:26)

# loss.py:21-23 / :78-80
CLASS_WEIGHTS = (0.8373, 0.9180, 0.8660, 1.0345, 1.0166, 0.9969, 0.9754, 1.0489, 0.8786, 1.0023, 0.9539, 0.9843, 1.1116, 0.9037, 1.0865, 1.0955, 1.0865,
                 1.1529, 1.0507)


def _num_classes():
    try:
        import datasets
        return datasets.num_classes
    except Exception:
        from .network import NUM_CLASSES
        return NUM_CLASSES


def _ignore_label():
    try:
        import datasets
        return datasets.ignore_label
    except Exception:
        return IGNORE_LABEL


def _on_gpu(m):
    return m.cuda() if torch.cuda.is_available() else m


def class_weight_rows(targets, classes, upper_bound=1.0, norm=False, batch_weights=False):
    """calculate_weights (loss.py:136-146) for every image of int64 `targets` [n,H,W] -> float32 [n, classes]; batch_weights: the batch histogram in every row.
    GPU tensors: the HIP kernel, no host sync. CPU tensors: torch.bincount and the same expression in float64. Both bit-equal to the numpy expression."""
    if targets.is_cuda:
        from .hip import kernels as K
        return K.label_class_weights(targets, classes, upper_bound, norm, batch_weights)
    n = targets.shape[0]
    flat = targets.reshape(n, -1)
    counts = torch.stack([torch.bincount(r[(r >= 0) & (r < classes)], minlength=classes) for r in flat]).to(torch.float64)
    if batch_weights:
        counts = counts.sum(0, keepdim=True).expand(n, -1)
    hist = counts / counts.sum(1, keepdim=True)
    spread = 1.0 / hist if norm else 1.0 - hist
    return (((hist != 0).to(torch.float64) * upper_bound * spread) + 1).to(torch.float32)


class ImageBasedCrossEntropyLoss2d(nn.Module):
    """Image Weighted Cross Entropy Loss (loss.py:120-163): every image's class histogram gives its weight row, the loss is the sum over images of that image's
    weighted-mean NLL. `weight` is accepted and, as in the reference (whose forward overwrites it), not used. batch_weights: cfg.BATCH_WEIGHTING there."""

    def __init__(self, classes, weight=None, size_average=True, ignore_index=255, norm=False, upper_bound=1.0, batch_weights=False):
        super().__init__()
        logging.info("Using Per Image based weighted loss")
        self.num_classes = classes
        self.weight = weight
        self.size_average = size_average
        self.ignore_index = ignore_index
        self.norm = norm
        self.upper_bound = upper_bound
        self.batch_weights = batch_weights

    def class_weights(self, targets):
        return class_weight_rows(targets, self.num_classes, self.upper_bound, self.norm, self.batch_weights)

    def forward(self, inputs, targets):
        rows = self.class_weights(targets).to(inputs.dtype)
        lp = F.log_softmax(inputs, dim=1)
        loss = 0.0
        for i in range(inputs.shape[0]):
            loss = loss + F.nll_loss(lp[i:i + 1], targets[i:i + 1], weight=rows[i], reduction='mean', ignore_index=self.ignore_index)
        return loss


class CrossEntropyLoss2d(nn.Module):
    """Cross Entropy NLL Loss (loss.py:167-180)."""

    def __init__(self, weight=None, size_average=True, ignore_index=255):
        super().__init__()
        logging.info("Using Cross Entropy Loss")
        self.nll_loss = nn.NLLLoss(weight=weight, reduction='mean', ignore_index=ignore_index)
        self.logsoftmax = nn.LogSoftmax(dim=1)
        self.size_average = size_average

    @property
    def weight(self):
        return self.nll_loss.weight

    @property
    def ignore_index(self):
        return self.nll_loss.ignore_index

    def forward(self, inputs, targets):
        return self.nll_loss(self.logsoftmax(inputs), targets)


def _ce_weight(args):
    return torch.Tensor(list(CLASS_WEIGHTS)) if getattr(args, 'cls_wt_loss', False) else None


def get_loss(args):
    """loss.py:14-43 -> (criterion, criterion_val)."""
    if getattr(args, 'img_wt_loss', False):
        criterion = _on_gpu(ImageBasedCrossEntropyLoss2d(classes=_num_classes(), size_average=True, ignore_index=_ignore_label(),
                                                         upper_bound=getattr(args, 'wt_bound', 1.0), batch_weights=getattr(args, 'batch_weighting', False)))
    elif getattr(args, 'jointwtborder', False):
        raise NotImplementedError('--jointwtborder (relaxed-border labels, ImgWtLossSoftNLL) is not supported by pinthememory_amd.loss')
    else:
        criterion = _on_gpu(nn.CrossEntropyLoss(weight=_ce_weight(args), reduction='mean', ignore_index=_ignore_label()))
    criterion_val = _on_gpu(nn.CrossEntropyLoss(reduction='mean', ignore_index=_ignore_label()))
    return criterion, criterion_val


def get_loss_aux(args):
    """loss.py:71-88 -> criterion of the auxiliary head."""
    return _on_gpu(nn.CrossEntropyLoss(weight=_ce_weight(args), reduction='mean', ignore_index=_ignore_label()))
