"""zstdsharp_amd — MI355X (gfx950) zstd block compressor/decompressor behind ZstdSharp's one-shot API.

Host-side mirror of the reference's safe API (src/ZstdSharp/Compressor.cs, Decompressor.cs, ZstdException.cs,
ThrowHelper.cs): same member names in snake_case next to the original PascalCase, same argument meaning and
error behaviour, over the C ABI in include/zstd_mi355x.h.
"""
from .errors import ZstdException, ZSTD_ErrorCode
from .compressor import Compressor, content_cuts, content_cuts_digests, piece_digests
from .decompressor import Decompressor
from .dictbuilder import DictBuilder
from .decompressor import ZSTD_d_windowLogMax, ZSTD_d_refMultipleDDicts, ZSTD_rmd_refSingleDDict, ZSTD_rmd_refMultipleDDicts
from .dictionaries import CDict, DDict, get_dict_id_from_dict, get_dict_id_from_frame
from . import _ffi
from .batch import compress_batch, compress_batch_async, compress_pack, compress_pack_async, content_cuts_async, decompress_batch, decompress_batch_async, decompress_ranges_async, pack_ranges
from .seekable import read_seek_table
from .streams import CompressionStream, DecompressionStream, EndOfStreamException

__all__ = ["Compressor", "Decompressor", "ZSTD_d_windowLogMax", "ZSTD_d_refMultipleDDicts", "ZSTD_rmd_refSingleDDict", "ZSTD_rmd_refMultipleDDicts", "DictBuilder", "CDict", "DDict", "get_dict_id_from_dict", "get_dict_id_from_frame", "CompressionStream", "DecompressionStream", "EndOfStreamException", "ZstdException", "ZSTD_ErrorCode", "compress_batch", "compress_batch_async", "compress_pack", "compress_pack_async", "content_cuts_async", "decompress_batch", "decompress_batch_async", "decompress_ranges_async", "pack_ranges", "read_seek_table", "content_cuts", "content_cuts_digests", "piece_digests", "_ffi"]
