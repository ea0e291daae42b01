"""Objects that say they live on a GPU (__cuda_array_interface__) for the tests of the Python API that run without one,
and the replacements for guetzli_amd.device_arrays' two seams that hand such objects out."""
import numpy as np

SENTINEL = 7   # what a fresh "tensor" holds: whatever a call did not write still holds it afterwards


class FakeDeviceArray:
    """Over numpy memory: in the emulation that is device memory.  strides= (bytes; None: contiguous), shape= and
    stream= are what the interface says, whatever the array's own are."""

    def __init__(self, array, readonly=False, strides=None, shape=None, stream=None):
        self.array = array
        self.__cuda_array_interface__ = {"shape": shape or array.shape, "typestr": array.dtype.str, "data": (array.ctypes.data, readonly),
                                         "version": 3, "strides": strides, "stream": stream}


class FakeDeviceAddress:
    """An address only: never dereferenced."""
    PTR = 0x7F0000000000

    def __init__(self, shape, typestr="|u1", stream=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (self.PTR, False), "version": 3,
                                         "strides": None, "stream": stream}


def new_tensor(shape, dtype, ordinal):
    """device_arrays.new_tensor on numpy memory (numpy's types: no bfloat16 here), filled with SENTINEL."""
    return FakeDeviceArray(np.full(shape, SENTINEL, np.dtype(str(dtype))))


def upload(array, ordinal):
    """device_arrays.upload on numpy memory."""
    return FakeDeviceArray(np.ascontiguousarray(array))


def install(monkeypatch):
    from guetzli_amd import device_arrays
    monkeypatch.setattr(device_arrays, "new_tensor", new_tensor)
    monkeypatch.setattr(device_arrays, "upload", upload)
