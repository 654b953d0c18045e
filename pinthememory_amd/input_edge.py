"""Input edge of the training step: what sits between the reference's DataLoader and `net(x, gts=...)`.

The reference's DomainUniformConcatDataset (datasets/multi_loader.py:81-102) stacks one sample per source domain, so a batch
arrives as float32 `[B, D, 3, H, W]` images and int64 `[B, D, H, W]` label maps; train.py:297-307 merges the domain axis and
copies both to the GPU. ToTensor + Normalize (transforms/transforms.py:95-97, train-time `mean_std` of datasets/__init__.py)
ran on the host before that. Here the host hands over what the decoder produced -- uint8 pixels and uint8 train ids, 4x / 8x
fewer PCIe bytes -- in pinned memory; the copy runs on a side stream while the previous step computes, and ToTensor / Normalize /
the int64 widening are two small kernels on that same stream (`pm_image_u8_to_nhwc4`, `pm_labels_u8_to_i64`).

`SyntheticDomainSource` is the stand-in for the loader (no datasets in this build); `DevicePrefetcher` is the product part.

The photometric augmentation the reference's training scripts run per image on the host before ToTensor (`--color_aug 0.5 --gblur`, datasets/__init__.py:63-95;
the hard ColorJitter(0.8, 0.8, 0.8, 0.3) + blur of the meta-test domains, :128-144; RandomHorizontallyFlip) runs here on the uint8 pixels already in HBM
(`pm_augment_u8`, `pm_labels_u8_flip_to_i64`): `PhotometricAugment` draws the per-image parameters on the host, the prefetcher launches the kernels on its side stream.

In front of it, the joint transform of the same scripts -- RandomSizeAndCrop (transforms/joint_transforms.py:414-444: bicubic resize by a random scale, nearest for the
mask, pad, random crop) -- runs on the uint8 pixels in HBM too, for the crop window alone and with PIL's bytes (`pm_resample_crop_u8`): `GeometricAugment` draws scale
and crop origin. The reference's order is kept: joint transforms, image-only transforms, ToTensor.

And in front of that, the datasets' own label decoding -- the loop over `color_to_trainid` of datasets/gtav.py:440-445 (three whole-image compares per entry) and over
`trainid_to_trainid` / `id_to_trainid` of synthia.py:254-257 and cityscapes.py -- is a table lookup per pixel (`pm_labels_decode_u8`), and with a geometry a step of its
mask gather (`pm_resample_crop_decode_u8`: a per-pixel map commutes with a nearest gather, so only the crop window is decoded, to the same bytes). `LabelDecode` holds
the tables the datasets hand over.
"""
import torch

from .hip import kernels as K
from .hip import ops


class SyntheticDomainSource:
    """Endless `[B, D, H, W, 3]` uint8 images + `[B, D, H, W]` uint8 train ids (255 = ignore) in `n_buffers` rotating host buffers,
    pinned when a GPU is present. Deterministic in (seed, batch index): batch i is the same bytes on every run and every rank layout."""

    def __init__(self, batch, domains, size, n_buffers=3, seed=0, classes=19, static=False):
        h, w = (size, size) if isinstance(size, int) else size
        self.shape = (batch, domains, h, w)
        self.seed, self.classes, self.i, self.static = seed, classes, 0, static
        pin = torch.cuda.is_available()
        self.bufs = [(torch.empty((batch, domains, h, w, 3), dtype=torch.uint8, pin_memory=pin),
                      torch.empty((batch, domains, h, w), dtype=torch.uint8, pin_memory=pin)) for _ in range(n_buffers)]
        if static:                                                             # the ring is filled once and replayed (decode cost belongs to loader workers)
            for i, (img, lab) in enumerate(self.bufs):
                self.fill(i, img, lab)

    def bytes_per_batch(self):
        b, d, h, w = self.shape
        return b * d * h * w * 4

    def fill(self, i, img, lab):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        img.copy_(torch.randint(0, 256, img.shape, generator=g, dtype=torch.uint8))
        blocks = torch.randint(0, self.classes + 1, (self.shape[0], self.shape[1], (self.shape[2] + 15) // 16, (self.shape[3] + 15) // 16), generator=g)
        blocks[blocks == self.classes] = 255                                   # ignore_label regions (datasets/cityscapes_labels.py trainId 255)
        lab.copy_(blocks.repeat_interleave(16, 2).repeat_interleave(16, 3)[:, :, :self.shape[2], :self.shape[3]].to(torch.uint8))

    def __iter__(self):
        return self

    def __next__(self):
        img, lab = self.bufs[self.i % len(self.bufs)]
        if not self.static:
            self.fill(self.i, img, lab)
        self.i += 1
        return img, lab


class PhotometricAugment:
    """Per-image parameters of the device-side augmentation, drawn on the host with the DISTRIBUTIONS of the reference's pipeline (torchvision 0.10, which it pins):
    ColorJitter(brightness, contrast, saturation, hue) -- factors uniform in [max(0, 1 - b), 1 + b], hue uniform in [-h, h], the four ops in a uniformly random
    order -- applied as a whole with probability p (RandomApply); RandomGaussianBlur's sigma = 0.15 + U[0, 1) * 1.15 with `blur`; a horizontal flip with probability
    0.5 with `flip`. Images flagged `hard` (the meta-test domains of train.py:199-211, get_meta_transforms) always get the jitter, at the `hard` strengths.

    The STREAM of random numbers is this class's own, not torchvision's or `random`'s: image j since construction (counted across calls) draws from a host
    torch.Generator seeded with (seed, j). So the result depends on (seed, position of the image in the sequence of all sampled images) alone -- the same
    for the same seed and call sequence, and unchanged when the same images are sampled in calls of other sizes. `last` keeps the raw draws of the latest call."""

    def __init__(self, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.5, blur=True, flip=True, hard=(0.8, 0.8, 0.8, 0.3), seed=0):
        self.soft, self.hard = (brightness, contrast, saturation, hue), tuple(hard)
        assert all(v >= 0 for v in self.soft + self.hard) and self.soft[3] <= 0.5 and self.hard[3] <= 0.5, 'ColorJitter strengths: >= 0, hue <= 0.5'
        self.p, self.blur, self.flip, self.seed = p, blur, flip, seed
        self.count = 0          # images sampled so far
        self.last = None

    def sample(self, n, hard=None):
        """Host array of n pm_aug_image structs (K.aug_params); hard: one bool per image, or None for none."""
        hard = [False] * n if hard is None else [bool(h) for h in hard]
        assert len(hard) == n
        arr = K.aug_params(n)
        last = dict(applied=[], factors=[], hue=[], sigma=[], flip=[], order=[])
        for i in range(n):
            g = torch.Generator().manual_seed((self.seed * 1000003 + self.count + i) & 0x7fffffffffffffff)
            u = torch.rand(7, generator=g, dtype=torch.float64).tolist()
            order = torch.randperm(4, generator=g).tolist()
            b, c, s, h = self.hard if hard[i] else self.soft
            applied = hard[i] or u[0] < self.p
            factors = [max(0.0, 1.0 - v) + u[1 + k] * (1.0 + v - max(0.0, 1.0 - v)) for k, v in enumerate((b, c, s))]
            hue = -h + u[4] * 2.0 * h
            sigma = 0.15 + u[5] * 1.15 if self.blur else 0.0
            flip = self.flip and u[6] < 0.5
            enabled = sum(1 << k for k, v in enumerate((b, c, s, h)) if v > 0) if applied else 0      # a zero strength is torchvision's None: the op does not run
            K.set_aug_image(arr[i], order, enabled, flip, hue, factors[0], factors[1], factors[2], sigma)
            for k, v in zip(('applied', 'factors', 'hue', 'sigma', 'flip', 'order'), (applied, factors, hue, sigma, flip, order)):
                last[k].append(v)
        self.count += n
        self.last = last
        return arr


class GeometricAugment:
    """Per-image geometry of the device-side RandomSizeAndCrop (`pm_resample_crop_u8`), drawn on the host with the DISTRIBUTIONS of the reference's
    joint_transforms.RandomSizeAndCrop(crop_size, crop_nopad, scale_min, scale_max, ignore_index, pre_size) and its RandomCrop:
      scale_amt = (pre_size / shorter edge, or 1) * U[scale_min, scale_max];  w, h = int(W * scale_amt), int(H * scale_amt);
      crop_nopad=False: an axis shorter than the crop is padded on both sides by (t - size) // 2 + 1 (image 0, mask ignore_index);
      crop origin: a uniform integer in [0, w - tw] (inclusive, w the padded width); with a centroid (x, y) -- scaled to int(c * scale_amt) and, as in the reference,
      NOT shifted by the pad -- a uniform integer in [c - tw, c] clamped to [0, w - tw], so the crop covers the centroid wherever one fits.
    crop_nopad=True is served while the resized image holds the crop; the reference then shrinks the crop to the shorter edge and resamples it back through Resize,
    which this class does not do: NotImplementedError.

    The STREAM of random numbers is this class's own, as PhotometricAugment's: image j since construction (counted across calls) draws from a host torch.Generator
    seeded with (seed, j), so the result is the same for the same seed and sequence of images whatever the call sizes. `last` keeps the raw draws of the latest call."""

    def __init__(self, crop_size, scale_min=0.5, scale_max=2.0, pre_size=None, crop_nopad=False, ignore_index=255, seed=0):
        self.crop = (int(crop_size), int(crop_size)) if isinstance(crop_size, (int, float)) else (int(crop_size[0]), int(crop_size[1]))
        assert 0 < scale_min <= scale_max and min(self.crop) > 0 and 0 <= ignore_index <= 255
        self.scale_min, self.scale_max, self.pre_size, self.crop_nopad, self.ignore_index, self.seed = scale_min, scale_max, pre_size, crop_nopad, ignore_index, seed
        self.count = 0          # images sampled so far
        self.last = None

    def sample(self, sizes, centroids=None):
        """K.GeoParams for len(sizes) images. sizes: (H, W) per image; centroids: None, or per image None / (x, y) in source pixels (the dataset chooses them)."""
        n = len(sizes)
        centroids = [None] * n if centroids is None else list(centroids)
        assert len(centroids) == n
        th, tw = self.crop
        geo = K.GeoParams(n, self.crop, self.ignore_index)
        last = dict(u=[], scale=[], size=[], pad=[], origin=[], centroid=[])
        for i, (H, W) in enumerate(sizes):
            g = torch.Generator().manual_seed((self.seed * 1000003 + self.count + i) & 0x7fffffffffffffff)
            u = torch.rand(3, generator=g, dtype=torch.float64).tolist()
            scale = 1.0 if self.pre_size is None else self.pre_size / min(H, W)
            scale *= self.scale_min + (self.scale_max - self.scale_min) * u[0]      # random.uniform
            w, h = int(W * scale), int(H * scale)
            if w < 1 or h < 1:
                raise ValueError('image %d: %d x %d at scale %g has no pixel left' % (i, H, W, scale))
            if self.crop_nopad:
                if th > h or tw > w:
                    raise NotImplementedError('crop_nopad=True with a %d x %d image under a %d x %d crop: the reference shrinks the crop and resamples it through '
                                              'Resize, which the device path does not do' % (h, w, th, tw))
                pad_h = pad_w = 0
            else:
                pad_h = (th - h) // 2 + 1 if th > h else 0
                pad_w = (tw - w) // 2 + 1 if tw > w else 0
            max_x, max_y = w + 2 * pad_w - tw, h + 2 * pad_h - th
            c = None if centroids[i] is None else (int(centroids[i][0] * scale), int(centroids[i][1] * scale))
            if c is None:
                x1, y1 = min(int(u[1] * (max_x + 1)), max_x), min(int(u[2] * (max_y + 1)), max_y)
            else:                                                             # randint(c - t, c), then clamped into the image
                x1 = min(max_x, max(0, c[0] - tw + min(int(u[1] * (tw + 1)), tw)))
                y1 = min(max_y, max(0, c[1] - th + min(int(u[2] * (th + 1)), th)))
            p = geo.images[i]
            p.h_in, p.w_in, p.h, p.w, p.pad_h, p.pad_w, p.y1, p.x1 = int(H), int(W), h, w, pad_h, pad_w, y1, x1
            for k, v in zip(('u', 'scale', 'size', 'pad', 'origin', 'centroid'), (u, scale, (h, w), (pad_h, pad_w), (y1, x1), c)):
                last[k].append(v)
        self.count += n
        self.last = last
        return geo


class LabelDecode:
    """The label tables of the datasets behind one loader, for decoding raw masks on the device (`pm_labels_decode_u8`, `pm_resample_crop_decode_u8`) instead of in
    the per-image host loops of the reference's datasets. The package carries no table of its own: a dataset passes the dicts it already has --
      add_colors(gtav.color_to_trainid): {(r, g, b): train id}; a pixel whose colour is not listed, or is listed with 255 / -1, becomes ignore_index (gtav.py:440-445);
      add_ids(synthia.trainid_to_trainid / cityscapes.id_to_trainid): {id: train id}, unlisted ids unchanged, -1 stored as 255 (synthia.py:254-257)
    -- and gets the table's index back. A batch then names one table per image (-1 or None: the mask holds train ids already, channel 0 is passed through). Tables are
    built by the library's host builders and uploaded once per device."""

    def __init__(self, ignore_index=255):
        if not 0 <= int(ignore_index) <= 255:
            raise ValueError('ignore_index %r outside 0..255' % (ignore_index,))
        self.ignore_index = int(ignore_index)
        self.tables, self.kinds = [], []
        self._dev = {}          # device -> (uint8 tensor of the tables, event of its upload)

    def __len__(self):
        return len(self.tables)

    def _add(self, table, kind):
        self.tables.append(table)
        self.kinds.append(kind)
        self._dev.clear()
        return len(self.tables) - 1

    def add_colors(self, mapping):
        if not isinstance(mapping, dict) or not mapping:
            raise ValueError('add_colors takes a non-empty dict {(r, g, b): value}')
        for k, v in mapping.items():
            if not (isinstance(k, (tuple, list)) and len(k) == 3 and all(int(c) == c for c in k)) or int(v) != v:
                raise ValueError('colour entry %r: %r is not (r, g, b): integer' % (k, v))
        return self._add(K.label_table_colors(mapping, self.ignore_index), 'colors')

    def add_ids(self, mapping):
        if not isinstance(mapping, dict) or not mapping:
            raise ValueError('add_ids takes a non-empty dict {id: value}')
        for k, v in mapping.items():
            if isinstance(k, (tuple, list)) or int(k) != k or int(v) != v:
                raise ValueError('id entry %r: %r is not integer: integer' % (k, v))
        return self._add(K.label_table_ids(mapping), 'ids')

    def image_table(self, entries, n, channels):
        """One table index per image (-1 = pass-through) from `entries` (index, -1 or None each), checked on the host for what the device cannot report."""
        entries = list(entries)
        if len(entries) != n:
            raise ValueError('%d table entries for %d images' % (len(entries), n))
        out = []
        for i, e in enumerate(entries):
            e = -1 if e is None else int(e)
            if not -1 <= e < len(self.tables):
                raise ValueError('image %d: table %d, have %d' % (i, e, len(self.tables)))
            if e >= 0 and self.kinds[e] == 'colors' and channels != 3:
                raise ValueError('image %d: a colour table on a %d-channel label slab' % (i, channels))
            out.append(e)
        return out

    def device_tables(self, device):
        """The tables in device memory (uploaded at the first call per device), ready on the current stream."""
        device = torch.device(device)
        if device not in self._dev:
            ev = torch.cuda.Event()
            buf = K.upload_label_tables(self.tables, device)
            ev.record(torch.cuda.current_stream(device))
            self._dev[device] = (buf, ev)
        buf, ev = self._dev[device]
        torch.cuda.current_stream(device).wait_event(ev)
        return buf

    def decode(self, lab_d, entries):
        """Raw uint8 [N,H,W] or [N,H,W,3] masks on the device -> uint8 train ids [N,H,W]."""
        table = self.image_table(entries, lab_d.shape[0], 3 if lab_d.dim() == 4 else 1)
        return K.labels_decode_u8(lab_d, self.device_tables(lab_d.device), table)


def domain_entries(domain_tables, lead):
    """Table entry per merged image of a [B, D, ...] batch (image b * D + d takes domain_tables[d]); lead: the axes in front of H, W."""
    d = lead[-1] if len(lead) >= 2 else 1
    domain_tables = [None] * d if domain_tables is None else list(domain_tables)
    if len(domain_tables) != d:
        raise ValueError('%d domain_tables for %d domains' % (len(domain_tables), d))
    total = 1
    for v in lead:
        total *= v
    return [domain_tables[i % d] for i in range(total)]


def hard_flags(label_shape, hard_domains):
    """One bool per image of a [B, D, H, W] label batch after the domain axis merged into the batch (image b * D + d): is d one of hard_domains?"""
    if not hard_domains:
        return None
    lead = tuple(label_shape[:-2])
    d = lead[-1] if len(lead) >= 2 else 1
    total = 1
    for v in lead:
        total *= v
    return [(i % d) in hard_domains for i in range(total)]


def sample_geometry(geometry, image_shape, meta=None):
    """geometry.sample for a merged [N, Hs, Ws, 3] batch: per-image sizes and centroids from the source's third item (a dict), else every image fills its slab."""
    n, hs, ws = image_shape[0], image_shape[1], image_shape[2]
    meta = meta or {}
    return geometry.sample(meta.get('sizes') or [(hs, ws)] * n, meta.get('centroids'))


class DevicePrefetcher:
    """Keeps `depth` batches in flight: H2D of the uint8 buffers and the u8 -> NHWC4 float / int64 kernels run on a side stream, an
    event hands the result to the compute stream (`next()` makes the current stream wait on it; the host never blocks on the GPU
    except to keep the source from refilling a pinned buffer whose copy is still in flight). The raw uint8 device slots are only
    touched by the side stream, so its own order protects them; the converted tensors are handed over with `record_stream`.

    augment (a PhotometricAugment, default None = exactly the plain conversion): every batch is sampled for and augmented on the side stream, image and labels alike.
    hard_domains: indices on the D axis of the source's [B, D, ...] batches whose images get the hard augmentation (the meta-test domains); an attribute the caller may
    reassign between batches -- it is read when a batch is ISSUED, i.e. `depth` batches before that batch is returned.
    geometry (a GeometricAugment, default None = no geometry): every batch is resized, padded and cropped on the side stream first (`pm_resample_crop_u8`); the plain
    conversion or the augmentation then runs on the crop. The source may then yield a third item, a dict with per-image 'sizes' ((H, W): the image lies in the
    top-left corner of its slab) and / or 'centroids'; without it every image fills its slab.
    decode (a LabelDecode, default None = the masks hold train ids) with domain_tables (one entry per index of the D axis: a table index of `decode`, -1 or None for
    the pass-through): the source's masks are raw, [B, D, H, W] ids or [B, D, H, W, 3] colours (an id-coded domain of a mixed batch keeps its id in channel 0), and
    are decoded on the side stream -- inside the mask gather of the geometry where there is one (`pm_resample_crop_decode_u8`), else by `pm_labels_decode_u8` in front
    of the conversion. What follows sees decoded uint8 train ids."""

    def __init__(self, source, depth=1, device=None, augment=None, hard_domains=None, geometry=None, decode=None, domain_tables=None):
        assert torch.cuda.is_available(), 'the input edge stages into HBM: needs a GPU'
        self.src, self.depth = iter(source), depth
        self.host_ring = max(1, len(getattr(source, 'bufs', [])) or 1)          # pinned buffers the source rotates through
        self.dev = device or torch.device('cuda', torch.cuda.current_device())
        self.side = torch.cuda.Stream(device=self.dev)
        self.slots, self.copied, self.ready = [None] * (depth + 1), [], []
        self.n = 0
        self.augment, self.hard_domains, self.geometry = augment, hard_domains, geometry
        assert decode is not None or domain_tables is None, 'domain_tables without a LabelDecode'
        self.decode, self.domain_tables = decode, domain_tables
        for _ in range(depth):
            self._issue()

    def _issue(self):
        if len(self.copied) >= self.host_ring:
            self.copied.pop(0).synchronize()                                   # the buffer the source is about to refill has left the host
        item = next(self.src)
        img_h, lab_h = item[0], item[1]
        k = self.n % len(self.slots)
        self.n += 1
        h, w = img_h.shape[-3:-1]
        lead = tuple(img_h.shape[:-3])                                         # the axes that merge into the batch
        lab_tail = (h, w)
        if self.decode is not None:                                            # raw masks: [.., H, W] ids or [.., H, W, 3] colours
            lab_tail = (h, w, 3) if lab_h.dim() == img_h.dim() else (h, w)
            table = self.decode.image_table(domain_entries(self.domain_tables, lead), img_h.numel() // (h * w * 3), 3 if len(lab_tail) == 3 else 1)
        with torch.cuda.stream(self.side):
            if self.slots[k] is None:
                self.slots[k] = (torch.empty(img_h.reshape(-1, h, w, 3).shape, dtype=torch.uint8, device=self.dev),
                                 torch.empty(lab_h.reshape(-1, *lab_tail).shape, dtype=torch.uint8, device=self.dev))
            img_d, lab_d = self.slots[k]
            img_d.copy_(img_h.reshape(-1, h, w, 3), non_blocking=True)        # train.py:297-307: the domain axis merges into the batch
            lab_d.copy_(lab_h.reshape(-1, *lab_tail), non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.side)
            if self.geometry is not None:                                      # RandomSizeAndCrop first: what follows sees the crop
                geo = sample_geometry(self.geometry, img_d.shape, item[2] if len(item) > 2 else None)
                if self.decode is None:
                    img_d, lab_d = K.resample_crop_u8(img_d, lab_d, geo)
                else:                                                          # the masks are decoded in the gather
                    img_d, lab_d = K.resample_crop_decode_u8(img_d, lab_d, geo, self.decode.device_tables(self.dev), table)
            elif self.decode is not None:
                lab_d = K.labels_decode_u8(lab_d, self.decode.device_tables(self.dev), table)
            if self.augment is None:
                x = ops.nchw(K.image_u8_to_nhwc4(img_d))
                gt = K.labels_u8_to_i64(lab_d)
            else:
                params = K.upload_aug_params(self.augment.sample(img_d.shape[0], hard_flags(lead + (h, w), self.hard_domains)), self.dev)
                x = ops.nchw(K.augment_u8(img_d, params))
                gt = K.labels_u8_to_i64(lab_d, params)
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.copied.append(done)
        self.ready.append((x, gt, ev))

    def next(self):
        """(x, gts) of the oldest batch in flight, valid on the current stream; issues the copy of the one after."""
        x, gt, ev = self.ready.pop(0)
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(ev)
        x.record_stream(cur)
        gt.record_stream(cur)
        self._issue()
        return x, gt
