"""Drop-in boundary of /root/reference/loss.py: get_loss (:14-43), get_loss_aux (:71-88), ImageBasedCrossEntropyLoss2d (:120-163) and CrossEntropyLoss2d
(:167-180), without the reference's `datasets` / `config` imports.

    from pinthememory_amd.loss import get_loss, get_loss_aux

Inside the networks (network.deepv3plus.segmentation_loss) these criteria never see materialised logits: the fused up-sample + cross-entropy kernels take the
class weights (ops.upsample_wce), and the image-based criterion's weight rows come from the labels on the device (kernels.label_class_weights) -- the reference
computes them with numpy on the host every step (`targets.data.cpu().numpy()`, np.histogram(normed=True), which current numpy no longer accepts), a sync that
cannot be captured into a graph. Called directly on materialised logits (validation code does that) the classes compute the same loss from torch ops.

Relaxed-border training (`--jointwtborder`, ImgWtLossSoftNLL, loss.py:182-263): the border set of every pixel is one 32-bit word built on the device from the same
int64 labels the memory and the auxiliary head use (kernels.relax_border_bits; RelaxedBoundaryLossToTensor, transforms/transforms.py:99-148, does it on the host with
scipy), the class weights come from those words (kernels.relax_class_weights) and the networks run ops.upsample_relax. The reference's uint8 multi-hot target is
accepted too (relaxed_border_target writes it). Not built: the relax-off schedule (`--rlx_off_iter`) and ImgWtLossSoftNLL_by_epoch."""
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


def _strict_mask(strict):
    return sum(1 << int(c) for c in set(strict or ()))


def border_set_bits(labels, classes, border_window=1, strict=None, ignore_id=255):
    """int64 labels [n,H,W] -> int32 words [n,H,W], bit c = class c is in the (2 border_window + 1)^2 window around the pixel, bit `classes` = the ignore class
    (ignore_id, every other label outside [0, classes) and everything outside the image). A pixel whose own class is in `strict` keeps its one-hot. GPU tensors: the
    HIP kernel. CPU tensors: the same integer shifts in torch."""
    assert labels.dim() == 3 and 1 <= classes <= 31 and 0 <= border_window <= 3
    labels = labels.long()
    if 0 <= ignore_id < classes:
        labels = labels.masked_fill(labels == ignore_id, 255)
    if labels.is_cuda:
        from .hip import kernels as K
        return K.relax_border_bits(labels, classes, border_window, _strict_mask(strict))
    b = border_window
    cls = torch.where((labels >= 0) & (labels < classes), labels, torch.full_like(labels, classes))
    hot = torch.ones_like(cls) << cls
    H, W = cls.shape[1:]
    padded = F.pad(hot, (b, b, b, b), value=1 << classes)
    bits = torch.zeros_like(hot)
    for i in range(2 * b + 1):
        for j in range(2 * b + 1):
            bits |= padded[:, i:i + H, j:j + W]
    if strict:
        bits = torch.where(((_strict_mask(strict) >> cls) & 1).bool(), hot, bits)
    return bits.to(torch.int32)


def multihot_bits(target):
    """the reference's uint8 target [n, classes + 1, H, W] (non-zero = set) -> the words of border_set_bits"""
    assert target.dim() == 4 and target.shape[1] <= 32
    if target.is_cuda:
        from .hip import kernels as K
        return K.multihot_to_bits(target.to(torch.uint8))
    shifts = torch.arange(target.shape[1]).view(1, -1, 1, 1)
    return ((target != 0).long() << shifts).sum(1).to(torch.int32)


def relaxed_border_target(labels, classes, border_window=1, strict=None, ignore_id=255):
    """RelaxedBoundaryLossToTensor (transforms/transforms.py:99-148) without scipy: labels [H,W] or [n,H,W] (any integer type, device or CPU) -> the reference's
    uint8 multi-hot [classes + 1, H, W] or [n, classes + 1, H, W], byte for byte (scipy's shift with order 3 and a constant fill is the integer shift on integers)."""
    single = labels.dim() == 2
    bits = border_set_bits(labels.unsqueeze(0) if single else labels, classes, border_window, strict, ignore_id)
    shifts = torch.arange(classes + 1, device=bits.device).view(1, -1, 1, 1)
    out = ((bits.unsqueeze(1) >> shifts) & 1).to(torch.uint8)
    return out[0] if single else out


def border_weight_rows(bits, classes, upper_bound=1.0, norm=False, batch_weights=False):
    """ImgWtLossSoftNLL.calculate_weights (loss.py:208-220) for every image of int32 words [n,H,W] -> float32 [n, classes]: hist = pixels whose set holds the class
    / set bits of the image (the ignore bit included), then class_weight_rows' expression in float64, the ignore entry dropped. An image without a set bit: ones.
    GPU tensors: the HIP kernel, no host sync; CPU: torch. Both bit-equal to the numpy expression."""
    if bits.is_cuda:
        from .hip import kernels as K
        return K.relax_class_weights(bits.contiguous(), classes, upper_bound, norm, batch_weights)
    n = bits.shape[0]
    shifts = torch.arange(classes + 1).view(1, -1, 1)
    counts = ((bits.reshape(n, 1, -1) >> shifts) & 1).sum(2).to(torch.float64)
    if batch_weights:
        counts = counts.sum(0, keepdim=True).expand(n, -1)
    total = counts.sum(1, keepdim=True)
    hist = counts / total
    spread = 1.0 / hist if norm else 1.0 - hist
    rows = ((hist != 0).to(torch.float64) * upper_bound * spread) + 1
    return torch.where(total == 0, torch.ones_like(rows), rows)[:, :classes].to(torch.float32)


class ImgWtLossSoftNLL(nn.Module):
    """Relax Loss (loss.py:193-263). forward(inputs, target): target is the reference's uint8 multi-hot [n, classes + 1, H, W] or int64 labels [n, H, W], from
    which the border sets are built here (border_window = cfg.BORDER_WINDOW, strict_border_classes = cfg.STRICTBORDERCLASS). Per pixel with S the real classes of
    its set: - mean(w over S) log(sum of softmax over S); image i: sum / (pixels with a set + 1); batch: mean over images. `weights` is accepted and, as in the
    reference, not used; batch_weights: cfg.BATCH_WEIGHTING. Classes outside a pixel's set contribute nothing (the reference's 0 * log p is NaN once p underflows)."""

    def __init__(self, classes, ignore_index=255, weights=None, upper_bound=1.0, norm=False, batch_weights=False, border_window=1, strict_border_classes=None):
        super().__init__()
        logging.info("Using Relaxed-border soft NLL loss")
        self.weights = weights
        self.num_classes = classes
        self.ignore_index = ignore_index
        self.upper_bound = upper_bound
        self.norm = norm
        self.batch_weights = batch_weights
        self.border_window = border_window
        self.strict_border_classes = list(strict_border_classes) if strict_border_classes else None

    def border_bits(self, target):
        if target.dim() == 4:
            assert target.shape[1] == self.num_classes + 1, 'expected a [n, %d, H, W] multi-hot target, got %s' % (self.num_classes + 1, tuple(target.shape))
            return multihot_bits(target)
        return border_set_bits(target, self.num_classes, self.border_window, self.strict_border_classes, self.ignore_index)

    def class_weights(self, bits):
        return border_weight_rows(bits, self.num_classes, self.upper_bound, self.norm, self.batch_weights)

    def forward(self, inputs, target):
        from .hip import ops
        bits = self.border_bits(target)
        return ops.relaxed_soft_nll(inputs, bits, self.class_weights(bits))


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
        # The reference reads both companions of the flag whenever it is set (config.py:126-130) and fails on a namespace without them. A driver that does not
        # carry them was written for a package without this criterion: it is told so instead of being handed a border window it never chose.
        missing = [f for f in ('strict_bdr_cls', 'rlx_off_iter') if not hasattr(args, f)]
        if missing:
            raise NotImplementedError('--jointwtborder (relaxed-border labels, ImgWtLossSoftNLL) needs its companion flags as the reference\'s train.py defines '
                                      'them (strict_bdr_cls: \'\' or "2,5", rlx_off_iter: -1); missing: %s' % ', '.join(missing))
        rlx_off = args.rlx_off_iter
        if rlx_off is not None and rlx_off > -1:
            raise NotImplementedError('--rlx_off_iter (REDUCE_BORDER_ITER, the relax-off schedule of --jointwtborder) is not supported by pinthememory_amd.loss: '
                                      'it marks boundaries with skimage.find_boundaries and rewrites the target in place')
        strict = args.strict_bdr_cls or ''
        strict = [int(i) for i in strict.split(',') if i.strip()] if isinstance(strict, str) else list(strict)
        criterion = _on_gpu(ImgWtLossSoftNLL(classes=_num_classes(), ignore_index=_ignore_label(), upper_bound=getattr(args, 'wt_bound', 1.0),
                                             batch_weights=getattr(args, 'batch_weighting', False), border_window=getattr(args, 'border_window', 1),
                                             strict_border_classes=strict or None))
    else:
        criterion = _on_gpu(nn.CrossEntropyLoss(weight=_ce_weight(args), reduction='mean', ignore_index=_ignore_label()))
    criterion_val = _on_gpu(nn.CrossEntropyLoss(reduction='mean', ignore_index=_ignore_label()))
    return criterion, criterion_val


def get_loss_aux(args):
    """loss.py:71-88 -> criterion of the auxiliary head."""
    return _on_gpu(nn.CrossEntropyLoss(weight=_ce_weight(args), reduction='mean', ignore_index=_ignore_label()))
