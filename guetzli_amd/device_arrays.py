"""Everything that looks at a device-resident object -- a torch tensor on a GPU, or an object that exports
__cuda_array_interface__ -- for the Python API (encoder.py, which keeps the policy of each public function): one
reader, one adapter for images that are read, one check for arrays that are written, and the two seams through which
the API allocates and uploads (called as attributes of this module, so one monkeypatch reaches every caller).  Pure
Python: it loads no library, and torch is imported where a torch tensor is met or made."""
from typing import NamedTuple

import numpy as np

DTYPES = ("uint8", "uint16", "float32", "float16", "bfloat16")
FLOAT_DTYPES = ("float32", "float16", "bfloat16")


class DeviceArray(NamedTuple):
    """What read() found: strides in elements; stream: the one the memory was made on (0: nothing to wait for);
    owner: the object that keeps the memory alive."""
    ptr: int
    shape: tuple
    strides: tuple
    dtype: str
    stream: int
    ordinal: int
    readonly: bool
    owner: object


class AlphaRefused(ValueError):
    """An image with an alpha channel (2 or 4 channels) where no background= says what to blend it over."""


def is_device_resident(x):
    """A torch tensor on a GPU, or any object that exports __cuda_array_interface__."""
    return bool(getattr(x, "is_cuda", False)) or hasattr(x, "__cuda_array_interface__")


def _names(dtypes):
    return ", ".join(dtypes[:-1]) + " or " + dtypes[-1]


def read(x, device, what, dtypes=DTYPES, error=TypeError):
    """The DeviceArray of `x`, which the caller knows as the parameter `what`.  Refused, in this order: an object that is
    not device-resident (TypeError), a tensor on another device than `device` (None: wherever it is), byte strides that
    are no multiple of the element size, a dtype outside `dtypes` (None: the caller judges it) as an `error`."""
    if getattr(x, "is_cuda", False):   # a torch tensor
        import torch
        ordinal = x.device.index if x.device.index is not None else torch.cuda.current_device()
        if device is not None and device != ordinal:
            raise ValueError(f"{what} lives on device {ordinal}, device={device} was asked for")
        rec = DeviceArray(x.data_ptr(), tuple(x.shape), tuple(x.stride()), str(x.dtype).replace("torch.", ""),
                          torch.cuda.current_stream(x.device).cuda_stream, ordinal, False, x)
    elif hasattr(x, "__cuda_array_interface__"):
        cai = x.__cuda_array_interface__
        dt, shape = np.dtype(cai["typestr"]), tuple(cai["shape"])   # (numpy has no bfloat16: such arrays come as torch tensors)
        if cai.get("strides") is None:
            byte_strides = tuple(int(np.prod(shape[i + 1:], dtype=np.int64)) * dt.itemsize for i in range(len(shape)))
        else:
            byte_strides = tuple(cai["strides"])
        if any(b % dt.itemsize for b in byte_strides):
            raise ValueError(f"{what} has strides that are no multiple of the element size")
        # the interface's stream: None / absent = nothing to wait for; 1 = the legacy default stream, with which the
        # context's (blocking) streams synchronise by themselves: nothing to hand over; 2 = the per-thread default stream,
        # which orders itself against nobody: handed over as it is -- it is hipStreamPerThread's handle too, and it names the
        # stream of the thread that makes the call (process_many, whose calls run on other threads, refuses it)
        stream = cai.get("stream") or 0
        rec = DeviceArray(cai["data"][0], shape, tuple(b // dt.itemsize for b in byte_strides), dt.name,
                          0 if stream == 1 else stream, 0 if device is None else device, bool(cai["data"][1]), x)
    else:
        raise TypeError(f"{what} is not device-resident: a GPU tensor, or an object with __cuda_array_interface__")
    if dtypes is not None and rec.dtype not in dtypes:
        raise error(f"{what} has dtype {rec.dtype}: {_names(dtypes)}")
    return rec


def stream_or(stream, own):
    """The stream= of a public function where it is given, the array's own otherwise."""
    return own if stream is None else int(stream)


def alpha_address(ptr, offset, itemsize):
    """The address of the alpha sample of pixel (0, 0), `offset` elements from `ptr` -- 0 (opaque) for None."""
    if offset is None:
        return 0
    address = int(ptr) + int(offset) * itemsize
    if not address:
        raise ValueError("an alpha sample at address 0")
    return address


def _refuse_negative(strides):
    if min(strides) < 0:
        raise ValueError("negative strides (a flipped view): make it contiguous first")


# ---- arrays that are read ----
def _layout_strides(shape, strides, layout, background=None):
    """(w, h, (stride_y, stride_x, stride_c), alpha offset or None) of an image of `shape` with element `strides`:
    2-D is grey (the one value for all three channels), 3-D is "HWC" or "CHW" with 3 channels, 1 (grey) or -- only
    with background= -- 2 (grey + alpha) or 4 (RGBA).  layout=None takes whichever of the first / last dimension is
    3 and refuses a shape where both are; where neither is, whichever is 1 (with background=: 1, 2 or 4), by the same
    rule."""
    if len(shape) == 2:
        (h, w), (sy, sx) = shape, strides
        return w, h, (sy, sx, 0), None
    if len(shape) != 3:
        raise ValueError(f"an image has 2 or 3 dimensions, not {len(shape)}")
    need_background = f"shape {tuple(shape)}: pixels with alpha are blended only over a background that is named: background=(r, g, b)"
    if layout is None:
        first, last = shape[0] == 3, shape[2] == 3
        if not first and not last:
            counts = (1,) if background is None else (1, 2, 4)
            first, last = shape[0] in counts, shape[2] in counts
            if not first and not last:
                if background is None and (shape[0] in (2, 4) or shape[2] in (2, 4)):
                    raise AlphaRefused(need_background)
                raise ValueError(f"shape {tuple(shape)}: neither the first nor the last dimension is 3"
                                 + (", 1, 2 or 4" if background is not None else " or 1"))
        if first and last:
            raise ValueError(f"shape {tuple(shape)} is ambiguous: say layout='HWC' or layout='CHW'")
        layout = "CHW" if first else "HWC"
    if layout == "HWC":
        (h, w, ch), (sy, sx, sc) = shape, strides
    elif layout == "CHW":
        (ch, h, w), (sc, sy, sx) = shape, strides
    else:
        raise ValueError(f"layout {layout!r}: 'HWC', 'CHW' or None")
    if ch in (2, 4) and background is None:
        raise AlphaRefused(need_background)
    if ch not in (1, 2, 3, 4):
        raise ValueError(f"shape {tuple(shape)} has {ch} channels in layout {layout}, not 1, 2, 3 or 4")
    alpha = (ch - 1) * sc if ch in (2, 4) else None   # the last channel
    return w, h, (sy, sx, sc if ch >= 3 else 0), alpha


def source(rec, layout, background=None, outer=()):
    """(w, h, (stride_y, stride_x, stride_c) in elements, alpha offset or None) of the image that `rec` holds: see
    _layout_strides.  A stride of 0 (an expanded view) is read like any other; a negative one is refused, among `outer`
    (the strides of dimensions around the image) too.  AlphaRefused where the image has alpha and background is None."""
    w, h, strides, alpha = _layout_strides(rec.shape, rec.strides, layout, background)
    _refuse_negative(strides + tuple(outer) + (alpha or 0,))
    return w, h, strides, alpha


# ---- arrays that are written ----
def _strides_alias(strides, counts):
    """gz_device_output's test: with the dimensions ordered by stride, a stride smaller than the extent (stride *
    count) of the dimension before it, or smaller than 1, lets two elements share an address.  A dimension of one
    element does not count."""
    least = 1
    for stride, count in sorted(zip(strides, counts)):
        if count == 1:
            continue
        if stride < least:
            return True
        least = stride * count
    return False


def check_destination(rec, want, dtypes, what):
    """`rec` as something to fill with an array of shape `want`.  Refused, in this order: read-only memory, a dtype
    outside `dtypes` (TypeError), another shape, negative strides, strides under which two elements share an address."""
    if rec.readonly:
        raise ValueError(f"{what} is read-only (its __cuda_array_interface__ says so)")
    if rec.dtype not in dtypes:
        raise TypeError(f"{what} has dtype {rec.dtype}: {_names(dtypes)}")
    if rec.shape != tuple(want):
        raise ValueError(f"{what} has shape {rec.shape}, what it is to receive has shape {tuple(want)}")
    _refuse_negative(rec.strides)
    if _strides_alias(rec.strides, rec.shape):
        raise ValueError(f"{what} has strides {rec.strides} under which two of its elements share an address (an expanded view?)")
    return rec


def destination(x, want, dtypes, device, what):
    """The DeviceArray of `x`, which is to be filled with an array of shape `want`: read()'s refusals (not
    device-resident, another device), then check_destination's."""
    return check_destination(read(x, device, what, dtypes=None), want, dtypes, what)


def image_shape(w, h, layout):
    if layout not in ("HWC", "CHW"):
        raise ValueError(f"layout {layout!r}: 'HWC' or 'CHW'")
    return (h, w, 3) if layout == "HWC" else (3, h, w)


def guess_layout(shape):
    """The layout of a destination for w x h x 3 samples: [3][h][w] where only the first dimension is 3, [h][w][3] otherwise."""
    return "CHW" if len(shape) == 3 and shape[0] == 3 and shape[2] != 3 else "HWC"


def image_destination(x, w, h, layout, dtypes, device, what):
    """destination() for w x h x 3 samples in `layout` (None: guess_layout of the shape read() found), with the strides
    as (y, x, c)."""
    if layout is not None:
        image_shape(w, h, layout)   # (a layout nobody knows is refused before the object is looked at)
    rec = read(x, device, what, dtypes=None)
    layout = layout or guess_layout(rec.shape)
    check_destination(rec, image_shape(w, h, layout), dtypes, what)
    return rec._replace(strides=rec.strides if layout == "HWC" else rec.strides[1:] + rec.strides[:1])


def batch_destination(x, n, w, h, layout, dtypes, device, what):
    """destination() for n images of w x h x 3 samples, [n] + image_shape(w, h, layout), with the strides as (n, y, x, c)."""
    shape = (n,) + image_shape(w, h, layout)
    rec = check_destination(read(x, device, what, dtypes=None), shape, dtypes, what)
    st = rec.strides
    return rec._replace(strides=st if layout == "HWC" else (st[0],) + st[2:] + st[1:2])


# ---- the seams: a fresh tensor, a host array brought over ----
def new_tensor(shape, dtype, ordinal):
    """A fresh torch tensor of `shape` and `dtype` (a name, or torch's own) on GPU `ordinal`, from the calling thread's
    current stream."""
    import torch
    name = str(dtype).replace("torch.", "")
    if name not in DTYPES:
        raise TypeError(f"dtype {dtype}: {_names(DTYPES)}")
    return torch.empty(tuple(shape), dtype=getattr(torch, name), device=f"cuda:{ordinal}")


def upload(array, ordinal):
    """Host samples -> a torch tensor on GPU `ordinal`, on the calling thread's current stream."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to(f"cuda:{ordinal}")
