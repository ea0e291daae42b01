"""guetzli_amd/device_arrays.py on its own: the reader of device-resident objects (the interface branch on fakes, the
torch branch on a stub), the adapter for images that are read, the check for arrays that are written, and the rule that
says when strides let two elements share an address.  No library is loaded, no GPU is needed.  CPU only."""
import itertools
import types

import numpy as np
import pytest

from fake_device import FakeDeviceAddress, FakeDeviceArray
from guetzli_amd import device_arrays as da


# ------------------------------------------------------------------ the reader: __cuda_array_interface__ ----
def test_interface_strides():
    rec = da.read(FakeDeviceAddress((2, 3, 4), "<u2"), None, "x")
    assert rec == (FakeDeviceAddress.PTR, (2, 3, 4), (12, 4, 1), "uint16", 0, 0, False, rec.owner)
    a = np.zeros((2, 5, 4), np.uint16)
    view = a[:, 1:4]
    rec = da.read(FakeDeviceArray(view, strides=view.strides), None, "x")
    assert (rec.ptr, rec.shape, rec.strides) == (view.ctypes.data, (2, 3, 4), (20, 4, 1))
    rec = da.read(FakeDeviceArray(a, strides=(0, 8, -2)), None, "x")     # the reader judges no stride but this:
    assert rec.strides == (0, 4, -1)
    with pytest.raises(ValueError, match="x has strides that are no multiple of the element size"):
        da.read(FakeDeviceArray(a, strides=(40, 3, 2)), None, "x")
    assert da.read(FakeDeviceArray(np.zeros((), np.uint8), shape=()), None, "x").strides == ()


def test_interface_readonly_ordinal_and_owner():
    a = np.zeros((2, 3), np.float32)
    fake = FakeDeviceArray(a, readonly=True)
    rec = da.read(fake, None, "x")
    assert rec.readonly is True and rec.owner is fake and rec.ordinal == 0
    rec = da.read(FakeDeviceArray(a), 2, "x")       # the interface names no device: the caller's word is taken
    assert rec.readonly is False and rec.ordinal == 2
    with pytest.raises(AttributeError):             # the record is immutable
        rec.ptr = 0


@pytest.mark.parametrize("said,read", [(None, 0), (0, 0), (1, 0), (2, 2), (0x5EED0, 0x5EED0)])
def test_interface_stream(said, read):
    assert da.read(FakeDeviceAddress((4, 4), stream=said), None, "x").stream == read


def test_interface_without_a_stream_entry():
    fake = FakeDeviceAddress((4, 4))
    del fake.__cuda_array_interface__["stream"], fake.__cuda_array_interface__["strides"]
    rec = da.read(fake, None, "x")
    assert rec.stream == 0 and rec.strides == (4, 1)


def test_interface_dtypes():
    for typestr, name in (("|u1", "uint8"), ("<u2", "uint16"), ("<f4", "float32"), ("<f2", "float16")):
        assert da.read(FakeDeviceAddress((2, 2), typestr), None, "x").dtype == name
    with pytest.raises(TypeError, match="rgb has dtype int32: uint8, uint16, float32, float16 or bfloat16"):
        da.read(FakeDeviceAddress((2, 2), "<i4"), None, "rgb")
    with pytest.raises(ValueError, match="image has dtype uint8: float32, float16 or bfloat16"):
        da.read(FakeDeviceAddress((2, 2), "|u1"), None, "image", dtypes=da.FLOAT_DTYPES, error=ValueError)
    assert da.read(FakeDeviceAddress((2, 2), "<i4"), None, "x", dtypes=None).dtype == "int32"   # (the caller judges it)


def test_what_is_not_device_resident():
    for x in (np.zeros((2, 2)), None, True, [1, 2]):
        assert not da.is_device_resident(x)
        with pytest.raises(TypeError, match="heatmap= is not device-resident"):
            da.read(x, None, "heatmap=")
        with pytest.raises(TypeError, match="out= is not device-resident"):
            da.destination(x, (2, 2), da.FLOAT_DTYPES, None, "out=")
    assert da.is_device_resident(FakeDeviceAddress((2, 2)))


# ------------------------------------------------------------------ the reader: torch tensors, on a stub ----
STREAM = 0x7EA0


def torch_stub(dtype, shape, strides, index):
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, device=types.SimpleNamespace(index=index), shape=shape,
                                 stride=lambda: strides, data_ptr=lambda: 0x1000)


@pytest.fixture()
def torch_streams(monkeypatch):
    import torch
    asked = []

    def current_stream(device):
        asked.append(device)
        return types.SimpleNamespace(cuda_stream=STREAM)
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    return asked


def test_torch_branch(torch_streams):
    import torch
    x = torch_stub(torch.float16, (2, 3, 4), (24, 4, 1), 1)
    rec = da.read(x, None, "x")
    assert rec == (0x1000, (2, 3, 4), (24, 4, 1), "float16", STREAM, 1, False, x) and rec.owner is x
    assert torch_streams == [x.device]               # the current stream of the tensor's own device
    assert da.read(x, 1, "x").ordinal == 1
    with pytest.raises(ValueError, match="distorted lives on device 1, device=0 was asked for"):
        da.read(x, 0, "distorted")
    x = torch_stub(torch.bfloat16, (5,), (1,), None)   # a device without an index: torch's current one
    rec = da.read(x, None, "x")
    assert (rec.dtype, rec.ordinal, rec.strides) == ("bfloat16", 3, (1,))
    assert da.read(x, 3, "x").ordinal == 3
    with pytest.raises(ValueError, match="x lives on device 3, device=0 was asked for"):
        da.read(x, 0, "x")
    with pytest.raises(TypeError, match="x has dtype int64"):
        da.read(torch_stub(torch.int64, (5,), (1,), 0), None, "x")
    dst = da.destination(torch_stub(torch.bfloat16, (2, 3), (8, 1), 0), (2, 3), da.FLOAT_DTYPES, 0, "distmap=")
    assert (dst.dtype, dst.strides, dst.stream) == ("bfloat16", (8, 1), STREAM)


# ------------------------------------------------------------------ images that are read ----
def record(view, base):
    """The DeviceArray of a numpy view, with addresses counted in elements from the start of `base`."""
    size = base.itemsize
    return da.DeviceArray((view.ctypes.data - base.ctypes.data) // size, view.shape, tuple(s // size for s in view.strides),
                          base.dtype.name, 0, 0, False, view)


def assert_addresses(image, layout, placed, base):
    """What source() returned addresses the samples of `image` (a numpy view, in `layout`; 2-D: grey), alpha included."""
    w, h, (sy, sx, sc), alpha = placed
    ptr = (image.ctypes.data - base.ctypes.data) // base.itemsize
    flat = base.ravel()
    px = image[..., None] if image.ndim == 2 else image if layout == "HWC" else image.transpose(1, 2, 0)
    assert px.shape[:2] == (h, w)
    ch = px.shape[2]
    colour = np.repeat(px[..., :1], 3, axis=2) if ch < 3 else px[..., :3]
    for y, x, c in itertools.product(range(h), range(w), range(3)):
        assert flat[ptr + y * sy + x * sx + c * sc] == colour[y, x, c], (y, x, c)
    assert (alpha is not None) == (ch in (2, 4))
    if alpha is not None:
        for y, x in itertools.product(range(h), range(w)):
            assert flat[ptr + alpha + y * sy + x * sx] == px[y, x, ch - 1], (y, x)


# shape -> the outcome under (layout None, "HWC", "CHW"), each without and with background=: the layout it is read in,
# or the refusal -- "ambiguous", or "alpha" (AlphaRefused)
SOURCES = {(1, 1): (("HWC", "HWC"), ("HWC", "HWC"), ("HWC", "HWC")),            # (2-D: grey, whatever layout= says)
           (1, 1, 3): (("HWC", "HWC"), ("HWC", "HWC"), ("CHW", "CHW")),         # (as CHW: one channel, 1 x 3)
           (3, 1, 1): (("CHW", "CHW"), ("HWC", "HWC"), ("CHW", "CHW")),
           (3, 2, 3): (("ambiguous", "ambiguous"), ("HWC", "HWC"), ("CHW", "CHW")),
           (2, 3, 1): (("HWC", "ambiguous"), ("HWC", "HWC"), ("alpha", "CHW")),  # (with background=, 2 may be grey + alpha)
           (2, 3, 2): (("alpha", "ambiguous"), ("alpha", "HWC"), ("alpha", "CHW")),
           (2, 3, 4): (("alpha", "ambiguous"), ("alpha", "HWC"), ("alpha", "CHW"))}


@pytest.mark.parametrize("shape", SOURCES, ids=str)
def test_source_shapes_layouts_and_background(shape):
    base = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) + 1
    for layout, outcomes in zip((None, "HWC", "CHW"), SOURCES[shape]):
        for background, outcome in zip((None, (1, 2, 3)), outcomes):
            case = (shape, layout, background)
            if outcome == "alpha":
                with pytest.raises(da.AlphaRefused, match="background="):
                    da.source(record(base, base), layout, background)
            elif outcome == "ambiguous":
                with pytest.raises(ValueError, match="ambiguous") as e:
                    da.source(record(base, base), layout, background)
                assert not isinstance(e.value, da.AlphaRefused), case
            else:
                assert_addresses(base, outcome, da.source(record(base, base), layout, background), base)


def test_source_refusals_that_are_no_alpha():
    rec = da.DeviceArray(0, (5, 6, 7), (42, 7, 1), "uint8", 0, 0, False, None)
    for layout, background in itertools.product((None, "HWC", "CHW"), (None, 0)):
        with pytest.raises(ValueError) as e:
            da.source(rec, layout, background)
        assert not isinstance(e.value, da.AlphaRefused)
    with pytest.raises(ValueError, match="layout 'WHC'"):
        da.source(rec._replace(shape=(5, 6, 3)), "WHC")
    for shape in ((4,), (1, 2, 3, 3)):
        with pytest.raises(ValueError, match="2 or 3 dimensions"):
            da.source(rec._replace(shape=shape, strides=(1,) * len(shape)), None)


def test_source_views():
    base = np.arange(5 * 6 * 3, dtype=np.uint16).reshape(5, 6, 3)
    crop = base[1:4, 2:4]                                   # (3, 2, 3): ambiguous without layout=
    assert_addresses(crop, "HWC", da.source(record(crop, base), "HWC"), base)
    assert da.source(record(crop, base), "HWC")[:3] == (2, 3, (18, 3, 1))
    planes = base[:2, :4].transpose(2, 0, 1)                # CHW strides over HWC memory
    placed = da.source(record(planes, base), None)
    assert placed == (4, 2, (18, 3, 1), None)
    assert_addresses(planes, "CHW", placed, base)
    rgba = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    placed = da.source(record(rgba.transpose(2, 0, 1), rgba), "CHW", (0, 0, 0))
    assert placed == (3, 2, (12, 4, 1), 3)
    assert_addresses(rgba.transpose(2, 0, 1), "CHW", placed, rgba)
    row = np.arange(4 * 3, dtype=np.float32).reshape(1, 4, 3)
    tall = np.broadcast_to(row, (2, 4, 3))                  # an expanded view: stride 0 is read like any other
    placed = da.source(record(tall, row), None)
    assert placed == (4, 2, (0, 3, 1), None)
    assert_addresses(tall, "HWC", placed, row)
    grey = np.broadcast_to(np.float32(5).reshape(1, 1), (3, 4))
    assert da.source(record(grey, grey), None) == (4, 3, (0, 0, 0), None)
    for flipped in (base[::-1], base[:, ::-1], base[:, :, ::-1]):
        with pytest.raises(ValueError, match="negative strides"):
            da.source(record(flipped, base), "HWC")
    with pytest.raises(ValueError, match="negative strides"):   # ... of dimensions around the image too
        da.source(record(base, base), "HWC", outer=(-90,))
    assert da.source(record(base[:, :, :1][:, :, ::-1], base), "HWC")[2] == (18, 3, 0)   # one channel: its stride is not used


def test_the_two_one_liners():
    assert da.stream_or(None, 5) == 5 and da.stream_or(0, 5) == 0 and da.stream_or(np.int64(9), 5) == 9
    assert da.alpha_address(1000, None, 4) == 0
    assert da.alpha_address(1000, 3, 4) == 1012 and da.alpha_address(1000, 0, 2) == 1000
    with pytest.raises(ValueError, match="address 0"):
        da.alpha_address(0, 0, 4)


# ------------------------------------------------------------------ arrays that are written ----
def fake(shape, dtype=np.float32, **kw):
    return FakeDeviceArray(np.zeros(shape, dtype), **kw)


@pytest.mark.parametrize("shape", [(1, 1), (1, 3), (2, 3), (2, 3, 3), (3, 2, 3), (2, 2, 3)], ids=str)
def test_destination(shape):
    n, size = len(shape), 4
    contiguous = np.zeros(shape, np.float32).strides
    dst = da.destination(fake(shape), shape, da.FLOAT_DTYPES, None, "out=")
    assert (dst.shape, dst.strides, dst.dtype) == (shape, tuple(s // size for s in contiguous), "float32")
    canvas = np.zeros(tuple(s + 3 for s in shape), np.float16)
    crop = canvas[tuple(slice(1, 1 + s) for s in shape)]    # a crop inside a larger array
    dst = da.destination(FakeDeviceArray(crop, strides=crop.strides), shape, da.FLOAT_DTYPES, None, "out=")
    assert dst.ptr == crop.ctypes.data and dst.strides == tuple(s // 2 for s in crop.strides)
    with pytest.raises(ValueError, match="out= has shape"):
        da.destination(fake(shape[::-1] + (1,)), shape, da.FLOAT_DTYPES, None, "out=")
    with pytest.raises(TypeError, match="out= has dtype uint8: float32, float16 or bfloat16"):
        da.destination(fake(shape, np.uint8), shape, da.FLOAT_DTYPES, None, "out=")
    with pytest.raises(ValueError, match="out= is read-only"):
        da.destination(fake(shape, readonly=True), shape, da.FLOAT_DTYPES, None, "out=")
    for axis in range(n):
        other = tuple(-s if i == axis else s for i, s in enumerate(contiguous))
        zero = tuple(0 if i == axis else s for i, s in enumerate(contiguous))
        if shape[axis] == 1:    # a dimension of one element: its stride does not count for the addresses
            assert da.destination(fake(shape, strides=zero), shape, da.FLOAT_DTYPES, None, "out=").strides[axis] == 0
            assert da.destination(fake(shape, strides=tuple(4 * 1000 if i == axis else s for i, s in enumerate(contiguous))),
                                  shape, da.FLOAT_DTYPES, None, "out=").strides[axis] == 1000
            continue
        with pytest.raises(ValueError, match="negative strides"):       # a flipped view
            da.destination(fake(shape, strides=other), shape, da.FLOAT_DTYPES, None, "out=")
        with pytest.raises(ValueError, match="share an address"):       # an expanded view
            da.destination(fake(shape, strides=zero), shape, da.FLOAT_DTYPES, None, "out=")
    if shape[-1] > 1 and n > 1 and shape[-2] > 1:   # rows that overlap: one element short of the row
        short = contiguous[:-2] + (contiguous[-2] - size, size)
        with pytest.raises(ValueError, match="share an address"):
            da.destination(fake(shape, strides=short), shape, da.FLOAT_DTYPES, None, "out=")


def test_destination_refuses_in_one_order():
    """Not device-resident, wrong device (the torch test), read-only, dtype, shape, negative strides, shared addresses."""
    want, everything = (2, 3), dict(readonly=True, strides=(-4, 0), shape=(3, 3))
    bad = FakeDeviceArray(np.zeros((3, 3), np.int32), **everything)
    with pytest.raises(ValueError, match="read-only"):
        da.destination(bad, want, da.FLOAT_DTYPES, None, "out=")
    del everything["readonly"]
    with pytest.raises(TypeError, match="dtype int32"):
        da.destination(FakeDeviceArray(np.zeros((3, 3), np.int32), **everything), want, da.FLOAT_DTYPES, None, "out=")
    with pytest.raises(ValueError, match="shape"):
        da.destination(FakeDeviceArray(np.zeros((3, 3), np.float32), **everything), want, da.FLOAT_DTYPES, None, "out=")
    with pytest.raises(ValueError, match="negative strides"):
        da.destination(FakeDeviceArray(np.zeros((3, 3), np.float32), strides=(-4, 0), shape=(2, 3)), want, da.FLOAT_DTYPES, None, "out=")
    with pytest.raises(ValueError, match="share an address"):
        da.destination(FakeDeviceArray(np.zeros((3, 3), np.float32), strides=(4, 0), shape=(2, 3)), want, da.FLOAT_DTYPES, None, "out=")


def test_image_destination_and_the_layout_guess():
    w, h = 5, 2
    assert da.guess_layout((h, w, 3)) == "HWC" and da.guess_layout((3, h, w)) == "CHW"
    assert da.guess_layout((3, h, 3)) == "HWC" and da.guess_layout((h, w)) == "HWC"
    assert da.image_shape(w, h, "HWC") == (h, w, 3) and da.image_shape(w, h, "CHW") == (3, h, w)
    for layout in (None, "WHC", "hwc"):
        with pytest.raises(ValueError, match="layout"):
            da.image_shape(w, h, layout)
    hwc, chw = np.zeros((h, w + 2, 3), np.uint8)[:, 1:1 + w], np.zeros((3, h + 1, w), np.uint16)[:, :h]
    for guess in (None, "HWC"):
        dst = da.image_destination(FakeDeviceArray(hwc, strides=hwc.strides), w, h, guess, da.DTYPES, None, "decoded=")
        assert (dst.ptr, dst.strides, dst.dtype) == (hwc.ctypes.data, (3 * (w + 2), 3, 1), "uint8")
    for guess in (None, "CHW"):
        dst = da.image_destination(FakeDeviceArray(chw, strides=chw.strides), w, h, guess, da.DTYPES, None, "decoded=")
        assert (dst.ptr, dst.strides, dst.shape) == (chw.ctypes.data, (w, 1, (h + 1) * w), (3, h, w))   # strides as (y, x, c)
    with pytest.raises(ValueError, match="decoded= has shape"):
        da.image_destination(FakeDeviceArray(chw, strides=chw.strides), w, h, "HWC", da.DTYPES, None, "decoded=")
    with pytest.raises(ValueError, match="layout 'WHC'"):     # before the object is looked at
        da.image_destination(None, w, h, "WHC", da.DTYPES, None, "out=")
    # [3][2][3]: HWC by the guess, 2 wide and 3 high -- and CHW, 3 wide and 2 high, only where the caller says so
    both = np.zeros((3, 2, 3), np.float32)
    assert da.image_destination(FakeDeviceArray(both), 2, 3, None, da.DTYPES, None, "x").strides == (6, 3, 1)
    assert da.image_destination(FakeDeviceArray(both), 3, 2, "CHW", da.DTYPES, None, "x").strides == (3, 1, 6)
    with pytest.raises(ValueError, match="shape"):
        da.image_destination(FakeDeviceArray(both), 3, 2, None, da.DTYPES, None, "x")
    with pytest.raises(ValueError, match="shape"):            # a 2-D destination is no image
        da.image_destination(fake((h, w)), w, h, None, da.DTYPES, None, "x")

    class Liar(FakeDeviceArray):   # the guess is made from the shape the reader returned, never from an attribute
        shape = (h, w, 3)
    assert da.image_destination(Liar(chw, strides=chw.strides), w, h, None, da.DTYPES, None, "x").strides == (w, 1, (h + 1) * w)


def test_strides_alias_is_sound():
    """Wherever two elements share an address, the rule says so.  (The converse does not hold, by design: the rule is the
    C ABI's nesting test, which refuses some harmless layouts.)"""
    cases = missed = 0
    for counts in itertools.product(range(1, 4), repeat=3):
        index = np.indices(counts).reshape(3, -1)
        for strides in itertools.product(range(8), repeat=3):
            cases += 1
            shared = len(np.unique(np.dot(strides, index))) < index.shape[1]
            if shared and not da._strides_alias(strides, counts):
                missed += 1
    assert cases == 27 * 512 and missed == 0
    assert not da._strides_alias((6, 3, 1), (2, 2, 3)) and not da._strides_alias((1, 2, 4), (2, 2, 3))
    assert da._strides_alias((3, 2, 1), (2, 2, 2))     # (harmless -- 0..6 are distinct -- and refused: not nested)


# ------------------------------------------------------------------ the seams ----
def test_new_tensor_refuses_other_dtypes_before_it_allocates():
    for dtype in ("int32", "float64", "bool"):
        with pytest.raises(TypeError, match="uint8, uint16, float32, float16 or bfloat16"):
            da.new_tensor((2, 2), dtype, 0)
