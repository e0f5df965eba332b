"""The steps on either side of the hot path: batched image/label input transforms on the device, the
pseudo-label PNG writer, and the `tgt_train.lst` round trip.

Reference surface mirrored (paths relative to the reference root):
  data_loader/segmentation/greenhouse.py:152-270           GreenhouseRGBDSegmentation: list parsing, PIL decode, transforms
  transforms/segmentation/data_transforms.py:15-66,191-212 Tensorize / Normalize / RandomFlip / Resize
  uest_seg_multi_os.py:720-728                             update_image_list
  uest_seg_multi_os.py:923-940                             per-image `Image.fromarray(label).save(png)` + path lists

What changes: the reference resizes and normalises one image at a time with Pillow on the host inside the DataLoader
(workers=0, uest_seg_multi_os.py:577) and blocks on a PNG encode per image in the label loop.  Here decoded uint8 images
go to the device as they are (3 B/pixel instead of 12) and `Preprocessor` does Resize + Normalize for the whole batch in two
launches with Pillow's exact fixed-point arithmetic; `LabelWriter` copies the merged uint8 maps back on a side stream into
pinned memory and native worker threads (C++ + zlib inside the library) encode/write the PNGs while the next batch is on the GPU.  Decoding the source JPEG /
PNG files stays with PIL on the host (file formats are outside the path).

The target set of a self-training run is static and only its labels change: `FrameStore` holds the decoded uint8 frames on the
device for the whole run, the label loops write their maps into it (`label_sink=store.put_labels`) and `ResidentTrainLoader` yields
the reference dataset's train batches from it (shuffled slots, `TrainPreprocessor` reading the store in place).
"""
import collections
import contextlib
import ctypes
import math
import os
import random
import struct
import zlib

import numpy as np
import torch

from ._native import FILTER_BILINEAR, FILTER_LANCZOS, TrainRec, check, lib

def host_cores():
    """Cores this process may run on (the affinity mask where the platform has one: a container's share, not the machine)."""
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def default_writer_workers(world=1):
    """PNG encoding is the host-side limit of the label loop (18 400 images/s with 8 workers against 15 000 from the GPU): most of
    this rank's share of the cores, at most 12."""
    return max(4, min(12, host_cores() // max(1, min(world, 8)) - 2))


MEAN = [0.485, 0.456, 0.406]      # transforms/classification/data_transforms.py:10-11
STD = [0.229, 0.224, 0.225]


# ------------------------------------------------------------------ list files
def update_image_list(tgt_train_lst, image_path_list, label_path_list, depth_path_list=None):
    """uest_seg_multi_os.py:720-728: one `image,label[,depth]` line per image."""
    with open(tgt_train_lst, 'w') as f:
        for idx in range(len(image_path_list)):
            if depth_path_list:
                f.write('%s,%s,%s\n' % (image_path_list[idx], label_path_list[idx], depth_path_list[idx]))
            else:
                f.write('%s,%s\n' % (image_path_list[idx], label_path_list[idx]))


def read_image_list(data_file, use_depth=False, root=None, check_files=True):
    """The list parsing of GreenhouseRGBDSegmentation.__init__ (greenhouse.py:162-197): comma-separated, right-stripped,
    every named file must exist (AssertionError like the reference's `assert os.path.isfile`)."""
    if root:
        data_file = os.path.join(root, data_file)
    images, masks, depths = [], [], []
    with open(data_file, 'r') as lines:
        for line in lines:
            parts = line.split(',')
            rgb, label = parts[0].rstrip(), parts[1].rstrip()
            if check_files:
                assert os.path.isfile(rgb), 'Not found : ' + rgb
                assert os.path.isfile(label), 'Not found : ' + label
            if use_depth:
                depth = parts[2].rstrip()
                if check_files:
                    assert os.path.isfile(depth), 'Not found : ' + depth
                depths.append(depth)
            images.append(rgb)
            masks.append(label)
    return images, masks, depths


# ------------------------------------------------------------------ device-side Resize + Normalize
class Preprocessor(object):
    """`Compose([Resize(size), Normalize() | Tensorize()])` (greenhouse.py:216-222) for a batch, on the device.

    size = (W, H) in PIL order like the reference's `size=(480, 256)`.  Call with uint8 tensors:
    rgb (N,Hs,Ws,3), label (N,Hs,Ws) or None, depth (N,Hs,Ws) or None, flip (N,) bool or None (RandomFlip's coin, drawn by
    the caller).  Host tensors are uploaded (pinned + non_blocking when possible).  Returns
    (rgb fp32 (N,3,H,W), label int64 (N,H,W) | None, depth fp32 (N,1,H,W) | None) on the device, bit-identical to the
    reference's PIL/torchvision pipeline."""

    def __init__(self, size=(480, 256), normalize=True, device='cuda'):
        self.size = size if isinstance(size, tuple) else (size, size)
        self.normalize = normalize
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('mspl_amd: Preprocessor runs on the GPU (no CPU path)')
        self.mean = torch.tensor(MEAN, dtype=torch.float32, device=self.device)
        self.std = torch.tensor(STD, dtype=torch.float32, device=self.device)
        self._tables = {}

    def _bilinear_tables(self, n_in, n_out):
        key = ('b', n_in, n_out)
        if key not in self._tables:
            k = lib.mspl_resample_ksize(n_in, n_out)
            if k <= 0:
                check(k)
            bounds = np.zeros((n_out, 2), np.int32)
            kk = np.zeros((n_out, k), np.int32)
            check(lib.mspl_resample_coeffs(n_in, n_out, bounds.ctypes.data, kk.ctypes.data))
            self._tables[key] = (torch.from_numpy(bounds).to(self.device), torch.from_numpy(kk).to(self.device), k)
        return self._tables[key]

    def _nearest_table(self, n_in, n_out):
        key = ('n', n_in, n_out)
        if key not in self._tables:
            idx = np.zeros(n_out, np.int32)
            check(lib.mspl_nearest_index(n_in, n_out, idx.ctypes.data))
            self._tables[key] = torch.from_numpy(idx).to(self.device)
        return self._tables[key]

    def _up(self, t, name, ndim):
        if t.dtype != torch.uint8 or t.dim() != ndim:
            raise RuntimeError('mspl_amd: %s must be a uint8 tensor with %d dims, got %s %s' % (name, ndim, t.dtype, tuple(t.shape)))
        return t.to(self.device, non_blocking=True).contiguous()

    def _bilinear(self, src, C, mean, std, flip, out=None):
        N, Hs, Ws = src.shape[:3]
        W, H = self.size
        yb, yk, ky = self._bilinear_tables(Hs, H)
        xb = xk = tmp = None
        kx = 0
        if Ws != W:
            xb, xk, kx = self._bilinear_tables(Ws, W)
            tmp = torch.empty((N, Hs, W, C), dtype=torch.uint8, device=self.device)
        if out is None:
            out = torch.empty((N, C, H, W), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (N, C, H, W) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise RuntimeError('mspl_amd: Preprocessor out= must be a contiguous CUDA float32 tensor of shape %s, got %s %s'
                               % ((N, C, H, W), tuple(out.shape), out.dtype))
        p = lambda t: None if t is None else t.data_ptr()
        check(lib.mspl_preprocess_u8_fwd(src.data_ptr(), N, Hs, Ws, C, H, W, p(xb), p(xk), kx, yb.data_ptr(), yk.data_ptr(), ky,
                                         p(mean), p(std), p(flip), p(tmp), out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream))
        return out

    def __call__(self, rgb, label=None, depth=None, flip=None, out=None):
        """out: optional destination of the image tensor (N,3,H,W) -- e.g. the static input slot of a captured label pass
        (PipelinedLabelPass.static_inputs()[next_lane]): the transform then writes the network input in place, no copy follows."""
        rgb = self._up(rgb, 'rgb', 4)
        if rgb.shape[3] != 3:
            raise RuntimeError('mspl_amd: rgb must be (N,H,W,3) uint8, got %s' % (tuple(rgb.shape),))
        N = rgb.shape[0]
        if flip is not None:
            flip = torch.as_tensor(flip).to(torch.uint8).to(self.device).contiguous()
            if flip.numel() != N:
                raise RuntimeError('mspl_amd: flip needs one flag per image')
        x = self._bilinear(rgb, 3, self.mean if self.normalize else None, self.std if self.normalize else None, flip, out)
        y = d = None
        if label is not None:
            label = self._up(label, 'label', 3)
            if label.shape[0] != N:
                raise RuntimeError('mspl_amd: label batch %d != image batch %d' % (label.shape[0], N))
            Hs, Ws = label.shape[1:]
            W, H = self.size
            y = torch.empty((N, H, W), dtype=torch.int64, device=self.device)
            check(lib.mspl_resize_label_fwd(label.data_ptr(), N, Hs, Ws, H, W, self._nearest_table(Hs, H).data_ptr(),
                                            self._nearest_table(Ws, W).data_ptr(), None if flip is None else flip.data_ptr(),
                                            y.data_ptr(), torch.cuda.current_stream().cuda_stream))
        if depth is not None:
            depth = self._up(depth, 'depth', 3)
            if depth.shape[0] != N:
                raise RuntimeError('mspl_amd: depth batch %d != image batch %d' % (depth.shape[0], N))
            d = self._bilinear(depth.unsqueeze(3), 1, None, None, flip)
        return x, y, d


# ------------------------------------------------------------------ device-side train augmentation
TrainDraw = collections.namedtuple('TrainDraw', 'sw sh pad_w pad_h i j flip')
TrainDraw.__doc__ = """One image's outcome of the train transforms' random draws: size after RandomScale (PIL order), RandomCrop's padding
per side and origin (row i, column j) in the padded image, RandomFlip's mirror."""


class TrainPreprocessor(object):
    """`Compose([RandomScale(scale)?, RandomCrop(size, ignore_idx) if crop else Resize(size), RandomFlip(), Normalize() | Tensorize()])`
    (transforms/segmentation/data_transforms.py:15-136,191-212) for a batch of decoded uint8 frames of one source size, on the device,
    bit-identical to Pillow + torchvision.  size = (W, H) in PIL order.  The reference pipelines:

        pipeline                                        scale        crop   ignore_idx
        Greenhouse RGB-D (greenhouse.py:211-219, uest)  (0.5, 2.0)   no     --
        CamVid (camvid.py:95-104)                       set          yes    4 or 12 (camvid.py:78-80)
        Cityscapes (cityscapes.py:109-117)              set          yes    255
        Greenhouse RGB (greenhouse.py:118-125)          None         yes    255

    (CamVid's Resize after its RandomCrop is Pillow's copy path: the crop is the size.)  `draw()` makes the reference's random draws
    with its own calls in its order; `__call__` uploads the per-image records (112 bytes each, pinned, asynchronous) and runs at most
    three launches.  Label remaps that datasets apply before their transforms (camvid.py:120-125, greenhouse.py:248-251) go in as
    `label_lut` or stay with the caller; image decoding stays with the caller (FrameStore.from_list does it once per run)."""

    def __init__(self, size=(480, 256), scale=(0.5, 2.0), crop=False, ignore_idx=255, normalize=True, device='cuda'):
        self.size = size if isinstance(size, tuple) else (size, size)
        if scale is not None and not isinstance(scale, tuple):
            scale = (scale, scale)                                  # RandomScale.__init__
        self.scale = scale
        self.crop = bool(crop)
        self.ignore_idx = int(ignore_idx)
        self.normalize = normalize
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('mspl_amd: TrainPreprocessor runs on the GPU (no CPU path)')
        self._mean = self._std = None
        self._tables = {}
        self._ws = None
        self._ws_dims = (0, 0, 0)

    # ---- host: the reference's random draws
    def draw(self, n, src_size, rng=random):
        """Records of n images of source size src_size = (W, H), drawn like the reference's transforms draw them for one image after
        the other: RandomScale one rng.random() (data_transforms.py:79-81), RandomCrop rng.randint(0, H'-th) then rng.randint(0, W'-tw)
        unless the padded size is the crop (:105-113, :117-118), RandomFlip one rng.random() < 0.5 (:54)."""
        w, h = src_size
        tw, th = self.size
        out = []
        for _ in range(n):
            sw, sh = w, h
            if self.scale is not None:
                lo, hi = self.scale
                rand_log_scale = math.log(lo, 2) + rng.random() * (math.log(hi, 2) - math.log(lo, 2))
                random_scale = math.pow(2, rand_log_scale)
                sw, sh = int(round(w * random_scale)), int(round(h * random_scale))
            pad_w = pad_h = i = j = 0
            if self.crop:
                pad_w = max(0, int((1 + tw - sw) / 2))
                pad_h = max(0, int((1 + th - sh) / 2))
                pw, ph = sw + 2 * pad_w, sh + 2 * pad_h
                if not (pw == tw and ph == th):
                    i = rng.randint(0, ph - th)
                    j = rng.randint(0, pw - tw)
            flip = rng.random() < 0.5
            out.append(TrainDraw(sw, sh, pad_w, pad_h, i, j, flip))
        return out

    # ---- device tables, built once per (in, out, filter)
    def _resample_table(self, n_in, n_out, filt):
        key = (filt, n_in, n_out)
        if key not in self._tables:
            k = lib.mspl_resample_ksize_filter(n_in, n_out, filt)
            if k <= 0:
                check(k)
            bounds = np.zeros((n_out, 2), np.int32)
            kk = np.zeros((n_out, k), np.int32)
            check(lib.mspl_resample_coeffs_filter(n_in, n_out, filt, bounds.ctypes.data, kk.ctypes.data))
            t = np.concatenate([np.array([k + 2], np.int32), np.concatenate([bounds, kk], 1).ravel()])
            self._tables[key] = torch.from_numpy(t).to(self.device)
        return self._tables[key].data_ptr()

    def _nearest_table(self, n_in, n_out):
        key = ('n', n_in, n_out)
        if key not in self._tables:
            idx = np.zeros(n_out, np.int32)
            check(lib.mspl_nearest_index(n_in, n_out, idx.ctypes.data))
            self._tables[key] = torch.from_numpy(idx).to(self.device)
        return self._tables[key].data_ptr()

    def _record(self, p, Hs, Ws, label_size, with_depth, scale_stage=True):
        """label_size: (Hl, Wl) of the label maps or None.  The label goes from its own size to (lsh, lsw) -- the frame's scaled size
        with a RandomScale stage (data_transforms.py:78-85), its own size without one -- and from there to the output."""
        W, H = self.size
        r = TrainRec()
        r.sh, r.sw, r.pad_h, r.pad_w, r.crop_i, r.crop_j, r.flip = p.sh, p.sw, p.pad_h, p.pad_w, p.i, p.j, int(bool(p.flip))
        if p.sh <= 0 or p.sw <= 0:
            raise RuntimeError('mspl_amd: TrainPreprocessor: scaled size %dx%d' % (p.sw, p.sh))
        if p.sw != Ws:
            r.scale_x = self._resample_table(Ws, p.sw, FILTER_LANCZOS)
            r.dscale_x = self._resample_table(Ws, p.sw, FILTER_BILINEAR) if with_depth else None
        if p.sh != Hs:
            r.scale_y = self._resample_table(Hs, p.sh, FILTER_LANCZOS)
            r.dscale_y = self._resample_table(Hs, p.sh, FILTER_BILINEAR) if with_depth else None
        if not self.crop:
            if p.sw != W:
                r.out_x = self._resample_table(p.sw, W, FILTER_BILINEAR)
            if p.sh != H:
                r.out_y = self._resample_table(p.sh, H, FILTER_BILINEAR)
        if label_size is not None:
            Hl, Wl = label_size
            lsh, lsw = (p.sh, p.sw) if scale_stage else (Hl, Wl)
            if lsw != Wl:
                r.near_x = self._nearest_table(Wl, lsw)
            if lsh != Hl:
                r.near_y = self._nearest_table(Hl, lsh)
            if not self.crop:
                if lsw != W:
                    r.near_out_x = self._nearest_table(lsw, W)
                if lsh != H:
                    r.near_out_y = self._nearest_table(lsh, H)
        return r

    def _up(self, t, name, ndim):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != ndim:
            raise RuntimeError('mspl_amd: %s must be a uint8 tensor with %d dims, got %s %s'
                               % (name, ndim, getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        return t.to(self.device, non_blocking=True).contiguous()

    def _out(self, t, shape, dtype, name):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError('mspl_amd: TrainPreprocessor out= %s must be a contiguous CUDA %s tensor of shape %s, got %s %s'
                               % (name, dtype, shape, t.dtype, tuple(t.shape)))
        return t

    def __call__(self, rgb, label=None, depth=None, params=None, out=None, slots=None, label_lut=None):
        """rgb (N,Hs,Ws,3), label (N,Hl,Wl), depth (N,Hs,Ws): uint8, host or device.  params: N records from draw() (None: draw()
        with the module-level `random`, as the reference's dataset does).  out: destination tensors -- the image tensor, or a tuple
        (x, y, d) whose entries may be None -- e.g. a train step's static input buffers.  Returns (x (N,3,H,W) fp32, y (N,H,W) int64
        | None, d (N,1,H,W) fp32 | None) on the device.

        The label maps may have a size of their own: RandomScale resizes them from it to the frame's scaled size
        (data_transforms.py:78-85), and a pipeline without RandomScale resizes them from it to `size` in one step (:191-212; with
        crop=True that case is refused: the reference would crop misaligned images).  slots: N slot numbers (a sequence or an int
        tensor on the host; a slot may repeat) -- the first three arguments are then STORES of M >= 1 frames (FrameStore.rgb /
        .labels / .depth) and output n comes from slot slots[n]: no staging copy.  label_lut: 256 uint8 values remapping the
        SOURCE label values in the gather (greenhouse.py:248-251, camvid.py:120-125); RandomCrop's fill is not remapped."""
        rgb = self._up(rgb, 'rgb', 4)
        if rgb.shape[3] != 3:
            raise RuntimeError('mspl_amd: rgb must be (N,H,W,3) uint8, got %s' % (tuple(rgb.shape),))
        M, Hs, Ws = rgb.shape[:3]
        if slots is None:
            N, slot_list = M, None
        else:
            slot_list = [int(v) for v in (slots.tolist() if hasattr(slots, 'tolist') else slots)]
            N = len(slot_list)
            if N == 0:
                raise RuntimeError('mspl_amd: TrainPreprocessor: an empty slot list')
        label_size = None
        if label is not None:
            label = self._up(label, 'label', 3)
            if label.shape[0] != M or 0 in label.shape:
                raise RuntimeError('mspl_amd: label shape %s does not match the image batch %s' % (tuple(label.shape), (M, Hs, Ws)))
            label_size = tuple(label.shape[1:])
        if depth is not None:
            depth = self._up(depth, 'depth', 3)
            if tuple(depth.shape) != (M, Hs, Ws):
                raise RuntimeError('mspl_amd: depth shape %s does not match the image batch %s' % (tuple(depth.shape), (M, Hs, Ws)))
        if params is None:
            params = self.draw(N, (Ws, Hs))
        if len(params) != N:
            raise RuntimeError('mspl_amd: %d records for a batch of %d images' % (len(params), N))
        W, H = self.size
        # label maps of the frame's size: the records alone say what is scaled, as they always have
        scale_stage = self.scale is not None or label_size in (None, (Hs, Ws))
        recs = (TrainRec * N)(*[self._record(p, Hs, Ws, label_size, depth is not None, scale_stage) for p in params])
        scaled = [(p.sh, p.sw) for p in params if (p.sh, p.sw) != (Hs, Ws)]
        ws = None
        if scaled:
            need = (max([Hs] + [s[0] for s in scaled]), max([Ws] + [s[1] for s in scaled]))
            if self.scale is not None:              # the whole range at once, so the workspace is allocated once
                need = (max(need[0], int(math.ceil(Hs * self.scale[1])) + 1), max(need[1], int(math.ceil(Ws * self.scale[1])) + 1))
            cn, ch, cw = self._ws_dims
            if N > cn or need[0] > ch or need[1] > cw:
                self._ws_dims = (max(N, cn), max(need[0], ch), max(need[1], cw))
                nbytes = lib.mspl_train_transform_workspace_bytes(self._ws_dims[0], self._ws_dims[1], self._ws_dims[2], 1)
                if nbytes < 0:
                    check(int(nbytes))
                self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            ws = self._ws
        max_sh, max_sw = (self._ws_dims[1], self._ws_dims[2]) if ws is not None else (max(p.sh for p in params), max(p.sw for p in params))
        if isinstance(out, torch.Tensor):
            out = (out, None, None)
        ox, oy, od = out if out is not None else (None, None, None)
        x = self._out(ox, (N, 3, H, W), torch.float32, 'x')
        y = None if label is None else self._out(oy, (N, H, W), torch.int64, 'y')
        d = None if depth is None else self._out(od, (N, 1, H, W), torch.float32, 'd')
        if self.normalize and self._mean is None:
            self._mean = torch.tensor(MEAN, dtype=torch.float32, device=self.device)
            self._std = torch.tensor(STD, dtype=torch.float32, device=self.device)
        if label_lut is not None:
            label_lut = torch.as_tensor(label_lut)
            if label_lut.dtype != torch.uint8 or label_lut.numel() != 256:
                raise RuntimeError('mspl_amd: label_lut must hold 256 uint8 values, got %s %s' % (label_lut.dtype, tuple(label_lut.shape)))
            label_lut = label_lut.to(self.device, non_blocking=True).contiguous()
        # one pinned block, one copy: the records, then the slot numbers (the records are 112 bytes each: int32 alignment holds)
        nrec = ctypes.sizeof(recs)
        host = torch.empty(nrec + (4 * N if slot_list is not None else 0), dtype=torch.uint8, pin_memory=True)
        ctypes.memmove(host.data_ptr(), ctypes.addressof(recs), nrec)
        if slot_list is not None:
            if min(slot_list) < -2 ** 31 or max(slot_list) >= 2 ** 31:     # the library checks [0, M); nothing may wrap before it
                raise RuntimeError('mspl_amd: TrainPreprocessor: slot numbers must fit int32')
            host[nrec:].view(torch.int32).copy_(torch.tensor(slot_list, dtype=torch.int32))
        dev = host.to(self.device, non_blocking=True)              # the allocator keeps `host` until the copy has run
        p = lambda t: None if t is None else t.data_ptr()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        mean, std = (self._mean, self._std) if self.normalize else (None, None)
        if slot_list is None and label_lut is None and label_size in (None, (Hs, Ws)):
            check(lib.mspl_train_transform_fwd(rgb.data_ptr(), p(label), p(depth), N, Hs, Ws, H, W, int(self.crop), self.ignore_idx,
                                               ctypes.addressof(recs), dev.data_ptr(), p(mean), p(std), p(ws), max_sh, max_sw,
                                               x.data_ptr(), p(y), p(d), stream))
            return x, y, d
        Hl, Wl = label_size if label_size is not None else (Hs, Ws)
        sh_ptr, sd_ptr = (host.data_ptr() + nrec, dev.data_ptr() + nrec) if slot_list is not None else (None, None)
        check(lib.mspl_train_transform_store_fwd(rgb.data_ptr(), p(label), p(depth), M, N, Hs, Ws, Hl, Wl, H, W, int(self.crop),
                                                 int(scale_stage), self.ignore_idx, ctypes.addressof(recs), dev.data_ptr(), sh_ptr, sd_ptr,
                                                 p(label_lut), p(mean), p(std), p(ws), max_sh, max_sw, x.data_ptr(), p(y), p(d), stream))
        return x, y, d


# ------------------------------------------------------------------ device-resident target set
def _decode_depth_u8(path):
    """The depth map as the reference's dataset reads it: cv2.imread(path, cv2.IMREAD_GRAYSCALE) (greenhouse.py:239).  Without OpenCV,
    8-bit single-channel files go through Pillow (the same bytes); any other file needs OpenCV's conversion and is refused."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        a = cv2.imread(path, cv2.IMREAD_GRAYSCALE)
        if a is None:
            raise RuntimeError('mspl_amd: FrameStore: OpenCV could not read the depth map %s' % path)
        return np.ascontiguousarray(a, dtype=np.uint8)
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != 'L':
            raise RuntimeError('mspl_amd: FrameStore: depth map %s has Pillow mode %r: without OpenCV (cv2) only 8-bit single-channel '
                               'files are read as the reference reads them' % (path, im.mode))
        return np.array(im, np.uint8)


class _StoreFrames(object):
    """FrameStore.frames(): consecutive slots as the tuples the label loop reads."""

    def __init__(self, store, batch_size):
        self.store, self.batch_size = store, int(batch_size)
        if self.batch_size <= 0:
            raise ValueError('mspl_amd: FrameStore.frames: batch_size %r' % (batch_size,))

    def __len__(self):
        return (len(self.store) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        s = self.store
        for a in range(0, len(s), self.batch_size):
            b = min(a + self.batch_size, len(s))
            if s.depth is not None:
                yield s.rgb[a:b], None, s.depth[a:b], s.names[a:b], None
            else:
                yield s.rgb[a:b], None, s.names[a:b], None


class FrameStore(object):
    """The decoded target set, held on the device for the whole run: the frames are static across the self-training
    rounds and only their labels change, so they are decoded once and every epoch of every round reads them in place.

        rgb     (M,Hs,Ws,3) uint8
        labels  (M,Hl,Wl) uint8, or None until the first labels arrive (from_list(with_labels=True), from_arrays, put_labels)
        depth   (M,Hs,Ws) uint8 or None
        names   the image paths, exactly as in the list file

    `frames(batch_size)` feeds the label pass, `put_labels` is its `label_sink`, ResidentTrainLoader trains from the store."""

    def __init__(self, rgb, labels=None, depth=None, names=None):
        M = rgb.shape[0]
        self.rgb, self.labels, self.depth = rgb, labels, depth
        self.names = [str(n) for n in names] if names is not None else ['%d' % k for k in range(M)]
        if len(self.names) != M:
            raise RuntimeError('mspl_amd: FrameStore: %d names for %d frames' % (len(self.names), M))
        self._slots = {}
        for k, n in enumerate(self.names):
            self._slots.setdefault(n, []).append(k)
        self.labelled = np.full(M, labels is not None, bool)       # host-side: which slots have received a label map

    def __len__(self):
        return self.rgb.shape[0]

    @property
    def device(self):
        return self.rgb.device

    def nbytes(self):
        return sum(t.numel() for t in (self.rgb, self.labels, self.depth) if t is not None)

    @staticmethod
    def _as_u8(t, name, shape_tail, M=None):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t))
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 + len(shape_tail):
            raise RuntimeError('mspl_amd: FrameStore: %s must be a uint8 array with %d dims, got %s %s'
                               % (name, 1 + len(shape_tail), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        if (M is not None and t.shape[0] != M) or any(w is not None and w != g for w, g in zip(shape_tail, t.shape[1:])):
            raise RuntimeError('mspl_amd: FrameStore: %s has shape %s, expected (%s, %s)'
                               % (name, tuple(t.shape), 'M' if M is None else M, ', '.join('*' if w is None else str(w) for w in shape_tail)))
        return t

    @classmethod
    def from_arrays(cls, rgb, labels=None, depth=None, names=None, device='cuda'):
        """For callers with their own decoder: rgb (M,Hs,Ws,3), labels (M,Hl,Wl), depth (M,Hs,Ws) uint8 arrays or tensors."""
        rgb = cls._as_u8(rgb, 'rgb', (None, None, 3))
        M, Hs, Ws = rgb.shape[:3]
        if M == 0:
            raise RuntimeError('mspl_amd: FrameStore: no frames')
        labels = None if labels is None else cls._as_u8(labels, 'labels', (None, None), M)
        depth = None if depth is None else cls._as_u8(depth, 'depth', (Hs, Ws), M)
        up = lambda t: None if t is None else t.to(device).contiguous()
        return cls(up(rgb), up(labels), up(depth), names)

    @classmethod
    def from_list(cls, list_file, use_depth=False, with_labels=True, root=None, max_bytes=8 << 30, workers=None, device='cuda'):
        """Decode the `image,label[,depth]` list once (read_image_list; greenhouse.py:232-245: frames `Image.open(p).convert('RGB')`,
        labels `np.array(Image.open(p), np.uint8)`, depth as _decode_depth_u8) on at most min(16, host_cores()) threads and upload.
        Every file must have the size of the first of its kind.  max_bytes: the device budget -- a larger set raises before anything
        is allocated there.  Dataset label remaps (greenhouse.py:248-251) are not applied here: pass them as ResidentTrainLoader's
        label_lut."""
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
        images, masks, depths = read_image_list(list_file, use_depth=use_depth, root=root, check_files=False)
        for kind, paths in (('image', images), ('label', masks if with_labels else []), ('depth', depths)):
            for p in paths:
                if not os.path.isfile(p):
                    raise FileNotFoundError('mspl_amd: FrameStore: %s file not found : %s' % (kind, p))
        M = len(images)
        if M == 0:
            raise RuntimeError('mspl_amd: FrameStore: %s lists no images' % list_file)

        def size_of(p):                                             # header only
            with Image.open(p) as im:
                return im.size[1], im.size[0]
        Hs, Ws = size_of(images[0])
        Hl, Wl = size_of(masks[0]) if with_labels else (0, 0)
        need = M * (Hs * Ws * (4 if use_depth else 3) + Hl * Wl)
        if need > max_bytes:
            raise RuntimeError('mspl_amd: FrameStore: %d frames of %dx%d need %d bytes on the device, max_bytes is %d'
                               % (M, Ws, Hs, need, max_bytes))
        rgb = np.empty((M, Hs, Ws, 3), np.uint8)
        lab = np.empty((M, Hl, Wl), np.uint8) if with_labels else None
        dep = np.empty((M, Hs, Ws), np.uint8) if use_depth else None

        def put(dst, k, a, path, kind):
            if a.shape != dst.shape[1:]:
                raise RuntimeError('mspl_amd: FrameStore: %s %s is %dx%d, the first one (%s) is %dx%d'
                                   % (kind, path, a.shape[1], a.shape[0], {'frame': images, 'label': masks, 'depth': depths}[kind][0],
                                      dst.shape[2], dst.shape[1]))
            dst[k] = a

        def decode(k):
            with Image.open(images[k]) as im:
                put(rgb, k, np.asarray(im.convert('RGB')), images[k], 'frame')
            if with_labels:
                with Image.open(masks[k]) as im:
                    a = np.array(im, np.uint8)
                if a.ndim != 2:
                    raise RuntimeError('mspl_amd: FrameStore: label %s is not a single-channel image (array shape %s)' % (masks[k], a.shape))
                put(lab, k, a, masks[k], 'label')
            if use_depth:
                put(dep, k, _decode_depth_u8(depths[k]), depths[k], 'depth')
        limit = min(16, host_cores())
        workers = limit if workers is None else max(1, min(int(workers), limit))
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(decode, range(M)))                        # the first error of a file, in list order, is raised here
        return cls.from_arrays(rgb, lab, dep, names=images, device=device)

    def put_labels(self, names, maps_u8, stream=None):
        """The `label_sink` of generate_pseudo_label*: the (n,Hl,Wl) uint8 device maps of `names` go into their slots by one
        device-to-device copy, issued on `stream` (or the current stream).  `labels` is allocated at the first call."""
        names = list(names)
        if (not isinstance(maps_u8, torch.Tensor) or maps_u8.dtype != torch.uint8 or maps_u8.dim() != 3 or maps_u8.shape[0] != len(names)
                or maps_u8.device != self.device):
            raise RuntimeError('mspl_amd: FrameStore.put_labels expects (n,Hl,Wl) uint8 maps on %s and n names, got %s %s / %d names'
                               % (self.device, getattr(maps_u8, 'dtype', type(maps_u8)), tuple(getattr(maps_u8, 'shape', ())), len(names)))
        dst, src = [], []
        for k, n in enumerate(names):
            if n not in self._slots:
                raise KeyError('mspl_amd: FrameStore.put_labels: %r is not a frame of this store' % (n,))
            for s in self._slots[n]:
                dst.append(s)
                src.append(k)
        if self.labels is None:
            # uninitialised on purpose: a fill on the current stream could land after a copy on `stream`; `labelled` says what is valid
            self.labels = torch.empty((len(self),) + tuple(maps_u8.shape[1:]), dtype=torch.uint8, device=self.device)
        elif tuple(maps_u8.shape[1:]) != tuple(self.labels.shape[1:]):
            raise RuntimeError('mspl_amd: FrameStore.put_labels: maps of %dx%d, the store holds %dx%d'
                               % (maps_u8.shape[2], maps_u8.shape[1], self.labels.shape[2], self.labels.shape[1]))
        if not dst:
            return
        ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        with ctx:
            if src == list(range(len(names))) and dst == list(range(dst[0], dst[0] + len(dst))):
                self.labels[dst[0]:dst[0] + len(dst)].copy_(maps_u8, non_blocking=True)           # consecutive slots: one plain copy
            else:
                idx = torch.tensor(dst, dtype=torch.int64).to(self.device, non_blocking=True)
                rows = maps_u8 if src == list(range(len(names))) else maps_u8[torch.tensor(src).to(self.device)]
                self.labels.index_copy_(0, idx, rows)
        self.labelled[dst] = True

    def frames(self, batch_size):
        """Iterable over consecutive slots yielding `(rgb_u8_view, None, names, None)` -- `(rgb_u8_view, None, depth_view, names,
        None)` with depth --: views, not copies, in the tuple shape the label loop reads (batch[0], batch[-2])."""
        return _StoreFrames(self, batch_size)


class ResidentTrainLoader(object):
    """The train loader of the self-training rounds over a FrameStore: yields the reference dataset's batch after default collation
    (greenhouse.py:267-270) with the tensors on the device --

        (images fp32 (n,3,H,W), labels int64 (n,H,W), names list, reg float64 (n,))            or, with use_depth,
        (images, labels, depth fp32 (n,1,H,W), names, reg)

    -- from one TrainPreprocessor call per batch that reads the store by slot.  The batch order is a real torch DataLoader's over
    the slot numbers (`shuffle`, `drop_last`, `sampler` are its arguments; a DistributedSampler gives each rank its shard), so the
    order and the torch RNG consumption are torch's own; the augmentation draws are `preprocessor.draw(n, (Ws, Hs))` once per batch:
    the reference's per-image draws in sampler order from the module-level `random`.  Everything runs on the current stream and
    nothing synchronises.  label_lut: 256 uint8 values, the dataset's label remap (greenhouse.py:248-251: lut[0] = 1)."""

    def __init__(self, store, preprocessor, batch_size, shuffle=True, drop_last=False, sampler=None, use_depth=False, reg_weight=0.0,
                 label_lut=None):
        from torch.utils.data import DataLoader
        if use_depth and store.depth is None:
            raise RuntimeError('mspl_amd: ResidentTrainLoader: use_depth with a store that holds no depth maps')
        self.store, self.preprocessor, self.use_depth, self.reg_weight = store, preprocessor, bool(use_depth), float(reg_weight)
        self.label_lut = None
        if label_lut is not None:
            lut = torch.as_tensor(label_lut)
            if lut.dtype != torch.uint8 or lut.numel() != 256:
                raise RuntimeError('mspl_amd: label_lut must hold 256 uint8 values, got %s %s' % (lut.dtype, tuple(lut.shape)))
            self.label_lut = lut.to(store.device).contiguous()
        self._index = DataLoader(range(len(store)), batch_size=batch_size, shuffle=bool(shuffle) and sampler is None, sampler=sampler,
                                 drop_last=drop_last, num_workers=0, collate_fn=list)
        self.batch_size, self.sampler = batch_size, self._index.sampler

    def __len__(self):
        return len(self._index)

    def __iter__(self):
        s, pre = self.store, self.preprocessor
        if s.labels is None:
            raise RuntimeError('mspl_amd: ResidentTrainLoader: the store has no labels yet (FrameStore.put_labels)')
        Hs, Ws = s.rgb.shape[1:3]
        for slots in self._index:
            slots = [int(k) for k in slots]
            if not s.labelled[slots].all():
                raise RuntimeError('mspl_amd: ResidentTrainLoader: slot %d has no label map yet'
                                   % [k for k in slots if not s.labelled[k]][0])
            x, y, d = pre(s.rgb, s.labels, s.depth if self.use_depth else None, params=pre.draw(len(slots), (Ws, Hs)), slots=slots,
                          label_lut=self.label_lut)
            names = [s.names[k] for k in slots]
            reg = torch.full((len(slots),), self.reg_weight, dtype=torch.float64, device=s.device)
            yield (x, y, d, names, reg) if self.use_depth else (x, y, names, reg)


# ------------------------------------------------------------------ label PNG writer
_PNG_SIG = b'\x89PNG\r\n\x1a\n'


def _chunk(typ, body):
    return struct.pack('>I', len(body)) + typ + body + struct.pack('>I', zlib.crc32(typ + body) & 0xffffffff)


def encode_png_gray8(arr, level=6):
    """8-bit single-channel PNG of a (H,W) uint8 array: what `Image.fromarray(label.astype(np.uint8)).save(path)` stores
    (uest_seg_multi_os.py:929-931) as far as a decoder can tell (mode 'L', same pixels).  Class-id maps are piecewise
    constant, so the Up filter (row minus the row above) turns them into mostly zeros before deflate."""
    arr = np.ascontiguousarray(arr)
    if arr.dtype != np.uint8 or arr.ndim != 2:
        raise ValueError('encode_png_gray8: expected a (H,W) uint8 array, got %s %s' % (arr.dtype, arr.shape))
    h, w = arr.shape
    raw = np.empty((h, w + 1), np.uint8)
    raw[:, 0] = 2
    raw[0, 1:] = arr[0]
    np.subtract(arr[1:], arr[:-1], out=raw[1:, 1:])              # uint8 wrap-around = PNG's modulo-256 arithmetic
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 0, 0, 0, 0)
    return _PNG_SIG + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(raw.tobytes(), level)) + _chunk(b'IEND', b'')


class LabelWriter(object):
    """Asynchronous replacement of the per-image save in the label loop (uest_seg_multi_os.py:923-940).

    `submit(names, labels)` takes the merged (N,H,W) uint8 maps as they leave the label pass (device tensor), starts a
    device->pinned-host copy of a snapshot on a side stream and returns at once (the caller may overwrite `labels`); native
    worker threads (mspl_png_writer_*, host C++ + zlib: no interpreter lock involved) wait for the copy, encode and write
    `<save_dir>/<image_name>.png` (image_name = basename without its extension, :924-926).  `close()` drains the queue and
    returns (image_path_list, label_path_list[, depth_path_list]) in submission order -- the arguments of
    update_image_list.  At most `max_inflight` batches are staged (pinned buffers are reused); beyond that submit() waits
    for the oldest one.  Also usable as a context manager."""

    def __init__(self, save_dir, workers=4, use_depth=False, level=3, max_inflight=None):
        self.save_dir = save_dir
        os.makedirs(save_dir, exist_ok=True)
        self.use_depth = use_depth
        self.level = level
        self.image_paths, self.label_paths, self.depth_paths = [], [], []
        self.max_inflight = max_inflight or 2 * max(1, workers)
        self._handle = lib.mspl_png_writer_create(max(1, workers), level)
        if not self._handle:
            raise RuntimeError('mspl_amd: could not start the PNG writer (workers=%r level=%r)' % (workers, level))
        self._free = {}             # shape -> pinned staging buffers not in use
        self._staged = 0            # staging buffers in existence
        self._inflight = []         # (ticket, staging buffer or None, keep-alive objects) in submission order
        self._stream = None

    def label_path(self, path_name):
        name = path_name.split('/')[-1]
        return '%s/%s.png' % (self.save_dir, name.rsplit('.', 1)[0])

    def _retire(self, block):
        """Collect finished batches (all of them when block is set to 'all', the oldest one when True)."""
        while self._inflight:
            ticket, host, _ = self._inflight[0]
            rc = lib.mspl_png_writer_poll(self._handle, ticket, 1 if block else 0)
            if rc == 0:
                return
            self._inflight.pop(0)
            if host is not None:
                self._free.setdefault(tuple(host.shape), []).append(host)
            if rc < 0:
                check(rc)
            if block is True:
                return

    def _staging(self, shape):
        self._retire(False)
        while True:
            pool = self._free.get(shape)
            if pool:
                return pool.pop()
            if self._staged < self.max_inflight:
                self._staged += 1
                return torch.empty(shape, dtype=torch.uint8, pin_memory=True)
            self._retire(True)                              # back-pressure: wait for the oldest batch in flight

    def warm(self, shape, count=None):
        """Allocate the staging buffers for (N,H,W) batches up front (first-use hipHostMalloc costs ~0.5 ms each)."""
        n = min(count or self.max_inflight, self.max_inflight) - self._staged
        bufs = [self._staging(tuple(shape)) for _ in range(max(0, n))]
        self._free.setdefault(tuple(shape), []).extend(bufs)

    def submit(self, names, labels, stream=None):
        """stream: issue the device -> host copy on THIS stream, straight from `labels` (no snapshot, no side stream).  For callers
        whose `labels` is only ever overwritten by work queued later on that same stream (a PipelinedLabelPass lane's static output
        and the lane's stream): stream order then protects the copy, and the copy needs no hardware queue of its own."""
        if labels.dtype != torch.uint8 or labels.dim() != 3 or labels.shape[0] != len(names):
            raise RuntimeError('mspl_amd: LabelWriter.submit expects (N,H,W) uint8 labels and N names, got %s %s / %d names'
                               % (labels.dtype, tuple(labels.shape), len(names)))
        if self._handle is None:
            raise RuntimeError('mspl_amd: LabelWriter is closed')
        paths = [self.label_path(n) for n in names]
        event, staged = None, None
        if labels.is_cuda and stream is not None:
            host = staged = self._staging(tuple(labels.shape))
            with torch.cuda.stream(stream):
                host.copy_(labels, non_blocking=True)
                event = torch.cuda.Event()
                event.record(stream)
        elif labels.is_cuda:
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=labels.device)
            host = staged = self._staging(tuple(labels.shape))
            snap = labels.clone()                          # contents as of submit(): the caller may reuse `labels` at once
            self._stream.wait_stream(torch.cuda.current_stream(labels.device))
            with torch.cuda.stream(self._stream):
                host.copy_(snap, non_blocking=True)
                event = torch.cuda.Event()
                event.record(self._stream)
            snap.record_stream(self._stream)
        else:
            host = labels.contiguous().clone()
        N, H, W = host.shape
        cpaths = (ctypes.c_char_p * N)(*[p.encode() for p in paths])
        ticket = lib.mspl_png_writer_submit(self._handle, host.data_ptr(), N, H, W, cpaths, None if event is None else event.cuda_event)
        if ticket < 0:
            check(int(ticket))
        self._inflight.append((ticket, staged, (host, event)))
        self.image_paths += list(names)
        self.label_paths += paths
        if self.use_depth:
            self.depth_paths += [n.replace('color', 'depth') for n in names]          # uest_seg_multi_os.py:936

    def close(self):
        if self._handle is not None:
            try:
                self._retire('all')
            finally:
                lib.mspl_png_writer_destroy(self._handle)
                self._handle = None
        if self.use_depth:
            return self.image_paths, self.label_paths, self.depth_paths
        return self.image_paths, self.label_paths

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
