"""Mirror of ZstdSharp.DictBuilder (S/DictBuilder.cs) over libzstd_mi355x.so: the fastCover trainer runs on the GPU."""
import ctypes

from . import _ffi
from .errors import ensure_zstd_success


class DictBuilder:
    """S/DictBuilder.cs:9-37."""

    DefaultDictCapacity = 112640        # used by the zstd utility by default

    @staticmethod
    def train_from_buffer(samples, dict_capacity: int = DefaultDictCapacity) -> bytes:
        """ZDICT_trainFromBuffer over the concatenated samples; raises ZstdException on a ZDICT error (EnsureZdictSuccess)."""
        lib = _ffi.load()
        samples = [bytes(s) for s in samples]
        flat = b"".join(samples)
        sizes = (ctypes.c_size_t * max(len(samples), 1))(*[len(s) for s in samples])
        src = ctypes.create_string_buffer(flat, max(len(flat), 1))
        dst = ctypes.create_string_buffer(max(dict_capacity, 1))
        n = ensure_zstd_success(lib, lib.ZDICT_trainFromBuffer(dst, dict_capacity, src, sizes, len(samples)))
        return dst.raw[:n]

    TrainFromBuffer = train_from_buffer
