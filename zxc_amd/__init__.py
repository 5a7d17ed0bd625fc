"""zxc_amd — MI355X-native ZXC block decode and LZ77 block encode.

The product is ``libzxc_mi355x.so`` (HIP kernels + C host API, built by
``__graft_entry__.build()`` from ``zxc_amd/csrc``); this package is only the thin
ctypes view of its C-ABI used by tests and bench.py. There is no Python or CPU
decoder behind it: if the library or a GPU is missing, calls raise.
"""
from .api import (ZxcError, Seekable, compress, decompress, get_decompressed_size, decode_blocks_device,  # noqa: F401
                  compress_device, compress_device_work_size, decompress_device, decompress_device_work_size,
                  frame_info_device, seekable_index_size, seekable_open_device, decompress_ranges_device_work_size,
                  decompress_ranges_device, dict_prepare_device, compress_dict_device, compress_dict_device_work_size,
                  decompress_dict_device, decompress_ranges_dict_device, decompress_batch_device_work_size,
                  decompress_batch_device, decompress_batch_dict_device, compress_batch_device_work_size, compress_batch_device,
                  compress_batch_dict_device, compress_pack_device_work_size, compress_pack_device, compress_pack_dict_device,
                  compress_append_device_work_size, compress_begin_device, compress_appendv_device_scratch_size,
                  compress_appendv_dict_device_scratch_size,
                  compress_append_dict_device_work_size, compress_begin_dict_device, CompressAppendSession, decompress_take_device_work_size, decompress_begin_device,
                  decompress_begin_dict_device, decompress_takev_device_scratch_size, DecompressTakeSession, lib, lib_path, JOB_DTYPE, RANGE_DTYPE, ITEM_DTYPE, IOV_DTYPE,
                  error_name, RANGEV_DTYPE, decompress_rangesv_device_work_size, decompress_rangesv_device,
                  decompress_rangesv_dict_device, shuffle_device, unshuffle_device, compress_shuffle_device_work_size,
                  compress_shuffle_device, decompress_shuffle_device_work_size, decompress_shuffle_device,
                  decompress_rangesv_shuffle_device_work_size, decompress_rangesv_shuffle_device, shufflev_device,
                  shufflev_device_scratch_size, compress_shufflev_device, compress_shufflev_device_work_size, unshufflev_device,
                  unshufflev_device_scratch_size, decompress_shufflev_device, decompress_shufflev_device_work_size)
from . import api  # noqa: F401  (stream_* helpers live there)
