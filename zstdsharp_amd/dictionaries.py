"""Digested dictionaries (include/zstd_mi355x.h "digested dictionaries"): ZSTD_CDict / ZSTD_DDict — a dictionary uploaded, validated and
indexed ONCE, then referenced by any number of Compressor / Decompressor objects and threads, and switched without another upload."""
from . import _ffi
from .compressor import _as_buffer


class _Digest:
    _create = _create_on = _free = _sizeof = _dict_id = None

    def __init__(self, handle):
        if not handle:
            raise ValueError(f"{type(self).__name__}: the dictionary was refused (a corrupt formatted dictionary), or no MI355X device or memory")
        self.handle = handle

    @property
    def dict_id(self) -> int:
        """the dictID of a formatted dictionary; 0 for raw content"""
        self._ensure_not_disposed()
        return getattr(self._lib, self._dict_id)(self.handle)

    @property
    def sizeof(self) -> int:
        """host plus device bytes held"""
        self._ensure_not_disposed()
        return getattr(self._lib, self._sizeof)(self.handle)

    def Dispose(self):
        """Free it.  As in libzstd the lifetime is the caller's: no Compressor / Decompressor may still reference it (RefCDict(None) first)."""
        if getattr(self, "handle", None):
            getattr(self._lib, self._free)(self.handle)
            self.handle = None

    dispose = close = Dispose

    def _ensure_not_disposed(self):
        if not self.handle:
            raise RuntimeError(f"ObjectDisposedException: {type(self).__name__}")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Dispose()


class CDict(_Digest):
    """ZSTD_createCDict: dict_bytes digested for compression at `level` (0 = 3), on `device` (None = where a fresh Compressor binds)."""
    _free, _sizeof, _dict_id = "ZSTD_freeCDict", "ZSTD_sizeof_CDict", "ZSTD_getDictID_fromCDict"

    def __init__(self, dict_bytes, level: int = 3, device: int = None):
        self._lib = _ffi.load()
        addr, n, keep = _as_buffer(dict_bytes if dict_bytes is not None else b"")
        self.level = int(level) if level else 3
        super().__init__(self._lib.ZSTD_createCDict(addr, n, int(level)) if device is None
                         else self._lib.ZSTDMI_createCDictOnDevice(addr, n, int(level), int(device)))


class DDict(_Digest):
    """ZSTD_createDDict: dict_bytes digested for decompression on `device`; a formatted dictionary's sequence tables are held ready-made."""
    _free, _sizeof, _dict_id = "ZSTD_freeDDict", "ZSTD_sizeof_DDict", "ZSTD_getDictID_fromDDict"

    def __init__(self, dict_bytes, device: int = None):
        self._lib = _ffi.load()
        addr, n, keep = _as_buffer(dict_bytes if dict_bytes is not None else b"")
        super().__init__(self._lib.ZSTD_createDDict(addr, n) if device is None else self._lib.ZSTDMI_createDDictOnDevice(addr, n, int(device)))


def get_dict_id_from_dict(dict_bytes) -> int:
    """ZSTD_getDictID_fromDict: the dictID of a formatted dictionary, 0 for raw content (no device is touched)"""
    addr, n, keep = _as_buffer(dict_bytes if dict_bytes is not None else b"")
    return _ffi.load().ZSTD_getDictID_fromDict(addr, n)


def get_dict_id_from_frame(src) -> int:
    """ZSTD_getDictID_fromFrame: the dictID a frame's header names, 0 if none (no device is touched)"""
    addr, n, keep = _as_buffer(src if src is not None else b"")
    return _ffi.load().ZSTD_getDictID_fromFrame(addr, n)
