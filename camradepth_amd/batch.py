"""GPU-side batch assembly: the tensor contract of the reference dataloader (src/data/dataloader.py:202-333) for the
radar configuration -- 7-channel input, inverse-normalised LiDAR ground truth and its zero-ignoring min-pool pyramid --
from raw device buffers (uint8 image as cv2 reads it, radar [H,W,3], radial velocity, LiDAR depth in metres).  File
decoding stays on the host; the image, the radar maps and the ground truth have device front ends of their own
(camradepth_amd.camera, .radar, .lidar), and the nearest-neighbour resizes of images and label maps are resize_image_nearest
and seg_targets below (no cv2 / skimage here).

Augmentation (`Augment`: random crop, horizontal flip, photometric jitter of the image) is this project's own -- the reference
trains without any -- and off unless asked for: INTEGRATION.md, "Augmentation"."""
import torch

from . import lib as L

_M64 = (1 << 64) - 1
_RANK_MUL = 0x632BE59BD9B4E019          # engine.py: one stream per data-parallel rank
_LEVELS = ("gt_half", "gt_quarter", "gt_eighth")


def _range(v, name, lowest_ok):
    """(lo, hi) of an optional jitter range -> (enabled, lo, hi)."""
    if v is None:
        return False, 1.0, 1.0
    lo, hi = (float(x) for x in v)
    if not (lo <= hi and lowest_ok(lo) and hi < float("inf")):
        raise L.CrdError(f"camradepth_amd.batch.Augment: bad {name} range {v!r}")
    return True, lo, hi


class Augment:
    """Per-sample random crop to `crop` = (h, w) (multiples of 32, no rescaling), horizontal flip with probability `hflip`, and --
    where a raw uint8 image is assembled -- gamma, brightness and per-channel colour gain drawn from the (lo, hi) ranges given.
    Every transform is off by default; Augment() changes nothing.  The draw is a pure function of (seed, rank, counter)
    (include/camradepth_hip.h: crd_augment_draw); `counter` is a host integer that advances by one per live draw and can be set,
    or saved and restored through state_dict() / load_state_dict(), to replay or resume a run."""

    def __init__(self, crop=None, hflip=0.0, gamma=None, brightness=None, colour=None, seed=0, rank=0):
        if crop is not None:
            crop = (int(crop[0]), int(crop[1]))
            if min(crop) <= 0 or crop[0] % 32 or crop[1] % 32:
                raise L.CrdError(f"camradepth_amd.batch.Augment: crop {crop} must be positive multiples of 32")
        if not 0.0 <= float(hflip) <= 1.0:
            raise L.CrdError(f"camradepth_amd.batch.Augment: hflip {hflip!r} is not a probability")
        self.crop, self.hflip = crop, float(hflip)
        self.gamma = _range(gamma, "gamma", lambda lo: lo > 0.0)
        self.brightness = _range(brightness, "brightness", lambda lo: lo >= 0.0)
        self.colour = _range(colour, "colour", lambda lo: lo >= 0.0)
        self.enable = (L.AUGMENT_GAMMA if self.gamma[0] else 0) | (L.AUGMENT_BRIGHTNESS if self.brightness[0] else 0) | \
                      (L.AUGMENT_COLOUR if self.colour[0] else 0)
        self.seed, self.rank = int(seed), int(rank)
        self.counter = 0

    def out_shape(self, H, W):
        """The shape a batch of H x W frames leaves with."""
        return self.crop if self.crop is not None else (H, W)

    def draw(self, B, H, W, counter=None, with_lut=False):
        """The device table int32 [B, 8] (y0, x0, flip, then the fp32 bits of gamma, brightness and three colour gains) for a batch of
        B frames H x W.  counter=None: a live draw at self.counter, which then advances by one; counter=k: draw k again, nothing
        advances.  with_lut: -> (table, the [B, 3, 256] image table made from it)."""
        live = counter is None
        k = self.counter if live else int(counter)
        h, w = self.out_shape(H, W)
        params = torch.empty(B, L.AUGMENT_WORDS, dtype=torch.int32, device="cuda")
        lut = torch.empty(B, 3, 256, device="cuda") if with_lut else None
        seed = (self.seed + self.rank * _RANK_MUL) & _M64
        L.check(L.load().crd_augment_draw(params.data_ptr(), L.ptr(lut), B, H, W, h, w, self.hflip, self.gamma[1], self.gamma[2],
                                          self.brightness[1], self.brightness[2], self.colour[1], self.colour[2], self.enable, seed,
                                          k & _M64, L.stream()), "crd_augment_draw")
        if live:
            self.counter += 1
        return (params, lut) if with_lut else params

    def lut(self, params):
        """The image table [B, 3, 256] of a given draw: the normalised value of every byte in every stored channel."""
        params = _check_params(params, params.shape[0])
        lut = torch.empty(params.shape[0], 3, 256, device=params.device)
        L.check(L.load().crd_augment_lut(params.data_ptr(), params.shape[0], self.enable, lut.data_ptr(), L.stream()), "crd_augment_lut")
        return lut

    def state_dict(self):
        return {"counter": self.counter}

    def load_state_dict(self, state):
        self.counter = int(state["counter"])


def _check_params(params, B):
    if not (torch.is_tensor(params) and params.is_cuda and params.dtype == torch.int32 and tuple(params.shape) == (B, L.AUGMENT_WORDS)):
        raise L.CrdError(f"an augmentation table is an int32 cuda tensor [{B}, {L.AUGMENT_WORDS}] (Augment.draw)")
    return params.contiguous()


def _pyramid_from_full(full, names):
    """The min-pool levels `names` of an inverse-normalised full map [B,1,h,w] (crd_gt_pyramid_from_full)."""
    B, _, h, w = full.shape
    maps = []
    for _ in names:
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        maps.append(torch.empty(B, 1, h, w, device=full.device))
    if maps:
        ptrs = [m.data_ptr() for m in maps] + [None] * (3 - len(maps))
        L.check(L.load().crd_gt_pyramid_from_full(full.data_ptr(), B, full.shape[2], full.shape[3], *ptrs, L.stream()),
                "crd_gt_pyramid_from_full")
    return dict(zip(names, maps))


def _label_outputs(B, h, w, dev):
    return (torch.empty(B, h, w, dtype=torch.int64, device=dev), torch.empty(B, h // 2, w // 2, dtype=torch.int64, device=dev))


def assemble_batch(img_u8, radar, rad_vel, gt_depth, max_depth=100.0, levels=3, augment=None, params=None, seg=None):
    """img_u8 [B,H,W,3] uint8, radar [B,H,W,3] fp32, rad_vel [B,H,W] fp32 or None, gt_depth [B,H,W] fp32 (metres), all on
    the GPU.  Returns {'image': [B,7,H,W], 'gt_full': [B,1,H,W], 'gt_half', 'gt_quarter'[, 'gt_eighth']} like
    camradepth_amd.synth.make_batch / the reference's batch dictionary.

    augment: an Augment -- the batch then has the crop's shape, every tensor cropped and flipped alike, the image through the sample's
    photometric table, the pyramid rebuilt from the augmented full map (one fused launch).  params: a table of Augment.draw to use in
    place of a live draw.  seg: uint8 labels [B,H,W] -> also 'final_seg' (= 'seg') [B,h,w] and 'intermediate_seg' [B,h/2,w/2], int64."""
    if not img_u8.is_cuda:
        raise L.CrdError("assemble_batch runs on the GPU (no CPU fallback)")
    lib = L.load()
    B, H, W, _ = img_u8.shape
    dev = img_u8.device
    img_u8, radar, gt_depth = img_u8.contiguous(), radar.contiguous().float(), gt_depth.contiguous().float()
    rv = rad_vel.contiguous().float() if rad_vel is not None else None
    names = ["gt_full", "gt_half", "gt_quarter", "gt_eighth"][:levels + 1]
    if params is not None and augment is None:
        raise L.CrdError("assemble_batch: params= is a draw of augment=, which gives the crop's shape and the enabled transforms")
    if augment is not None or seg is not None:
        augment = augment if augment is not None else Augment()
        h, w = augment.out_shape(H, W)
        if params is None:
            params, lut = augment.draw(B, H, W, with_lut=True)
        else:
            params = _check_params(params, B)
            lut = augment.lut(params)
        x = torch.empty(B, 7 if rv is not None else 6, h, w, device=dev)
        full = torch.empty(B, 1, h, w, device=dev)
        if seg is not None:
            if not seg.is_cuda or seg.dtype != torch.uint8 or tuple(seg.shape) != (B, H, W):
                raise L.CrdError(f"assemble_batch: seg is a uint8 cuda tensor [{B}, {H}, {W}]")
            seg = seg.contiguous()
        fseg, iseg = _label_outputs(B, h, w, dev) if seg is not None else (None, None)
        L.check(lib.crd_augment_assemble(img_u8.data_ptr(), radar.data_ptr(), L.ptr(rv), gt_depth.data_ptr(), L.ptr(seg), params.data_ptr(),
                                         lut.data_ptr(), B, H, W, h, w, float(max_depth), x.data_ptr(), full.data_ptr(), L.ptr(fseg),
                                         L.ptr(iseg), L.stream()), "crd_augment_assemble")
        out = {"image": x, "gt_full": full}
        out.update(_pyramid_from_full(full, names[1:]))
        if seg is not None:
            out.update({"seg": fseg, "final_seg": fseg, "intermediate_seg": iseg})
        return out
    x = torch.empty(B, 7 if rv is not None else 6, H, W, device=dev)
    L.check(lib.crd_assemble_input(img_u8.data_ptr(), radar.data_ptr(), rv.data_ptr() if rv is not None else None, B, H, W,
                                   float(max_depth), x.data_ptr(), L.stream()), "crd_assemble_input")
    maps, h, w = [], H, W
    for _ in names:
        maps.append(torch.empty(B, 1, h, w, device=dev))
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    ptrs = [m.data_ptr() for m in maps] + [None] * (4 - len(maps))
    L.check(lib.crd_gt_pyramid(gt_depth.data_ptr(), B, H, W, float(max_depth), *ptrs, L.stream()), "crd_gt_pyramid")
    out = {"image": x}
    out.update(dict(zip(names, maps)))
    return out


def augment_batch(batch, augment, params=None):
    """The geometry of `augment` (crop, flip; no photometric jitter: the image is normalised floats already) on a flat batch dictionary --
    camradepth_amd.synth.make_batch, runner.unpack_batch, assemble_batch: 'image' [B,C,H,W], 'gt_full', the pyramid levels present
    (rebuilt from the augmented full map), 'seg' / 'final_seg' int64 [B,H,W] and 'intermediate_seg'.  Tensors are moved to the GPU; other
    keys pass through.  params: a table of Augment.draw in place of a live draw."""
    image = batch["image"].cuda().float().contiguous()
    B, C, H, W = image.shape
    h, w = augment.out_shape(H, W)
    params = augment.draw(B, H, W) if params is None else _check_params(params, B)
    gt = batch["gt_full"].cuda().float().contiguous()
    if gt.numel() != B * H * W:
        raise L.CrdError(f"augment_batch: gt_full {tuple(gt.shape)} does not match the image {tuple(image.shape)}")
    names = [n for n in _LEVELS if n in batch]
    if names != list(_LEVELS[:len(names)]):
        raise L.CrdError(f"augment_batch: pyramid levels {names} (a level needs the one above it)")
    seg_key = "seg" if "seg" in batch else "final_seg" if "final_seg" in batch else None
    seg = batch[seg_key].cuda().long().contiguous() if seg_key else None
    if seg is not None and tuple(seg.shape) != (B, H, W):
        raise L.CrdError(f"augment_batch: labels {tuple(seg.shape)} do not match the image {tuple(image.shape)}")
    x = torch.empty(B, C, h, w, device=image.device)
    full = torch.empty(B, 1, h, w, device=image.device)
    fseg, iseg = _label_outputs(B, h, w, image.device) if seg is not None else (None, None)
    if "intermediate_seg" not in batch:
        iseg = None
    L.check(L.load().crd_augment_gather(image.data_ptr(), gt.data_ptr(), L.ptr(seg), params.data_ptr(), B, C, H, W, h, w, x.data_ptr(),
                                        full.data_ptr(), L.ptr(fseg), L.ptr(iseg), L.stream()), "crd_augment_gather")
    out = dict(batch)
    out.update({"image": x, "gt_full": full})
    out.update(_pyramid_from_full(full, names))
    for key in ("seg", "final_seg"):
        if key in batch:
            out[key] = fseg
    if iseg is not None:
        out["intermediate_seg"] = iseg
    return out


def resize_image_nearest(img_u8, size):
    """cv2.resize(image, size[::-1], interpolation=cv2.INTER_NEAREST) of dataloader.py:227 for a uint8 cuda batch
    [B,H,W,C]; size = (H_out, W_out) like args.image_dimension."""
    if not img_u8.is_cuda or img_u8.dtype != torch.uint8:
        raise L.CrdError("resize_image_nearest takes a uint8 cuda tensor [B,H,W,C] (no CPU fallback)")
    B, H, W, Cc = img_u8.shape
    out = torch.empty(B, size[0], size[1], Cc, dtype=torch.uint8, device=img_u8.device)
    L.check(L.load().crd_resize_nearest_u8(img_u8.contiguous().data_ptr(), B, H, W, Cc, out.data_ptr(), size[0], size[1], L.stream()),
            "crd_resize_nearest_u8")
    return out


def seg_targets(mseg_u8, rows=416, sizes=((416, 800), (208, 400))):
    """The two segmentation targets of dataloader.py:262-267 from uint8 cuda label maps [B,H,W]: the first `rows` rows,
    nearest-resized to each size (skimage order 0), as int64 -- {'final_seg', 'intermediate_seg'} of the batch dict."""
    if not mseg_u8.is_cuda or mseg_u8.dtype != torch.uint8:
        raise L.CrdError("seg_targets takes a uint8 cuda tensor [B,H,W] (no CPU fallback)")
    B, H, W = mseg_u8.shape
    src = mseg_u8.contiguous()
    outs = []
    for (h, w) in sizes:
        o = torch.empty(B, h, w, dtype=torch.int64, device=src.device)
        L.check(L.load().crd_resize_labels_nearest(src.data_ptr(), B, H, W, rows, o.data_ptr(), h, w, L.stream()),
                "crd_resize_labels_nearest")
        outs.append(o)
    return dict(zip(("final_seg", "intermediate_seg"), outs))
