"""Device ops on torch tensors, backed by the hand-written gfx950 kernels in
``brpc_amd/csrc/gpu/kernels.hip``. No fallback path: a CPU tensor or a
missing extension raises."""
from .crc32c import crc32c, crc32c_batch, crc32c_host, crc32c_packed  # noqa: F401
from .varint import varint_decode, varint_encode, varint_encode_host, varint_decode_host  # noqa: F401
from .copy import batched_copy, batched_copy_crc32c, batched_copy_crc32c_messages  # noqa: F401
from .pb import (pb_build_message, pb_build_records, pb_build_rows, pb_scan, pb_split_records,  # noqa: F401
                 pb_split_rows)
from .snappy import snappy_compress, snappy_compress_blocks, snappy_decompress, snappy_decompress_streams  # noqa: F401,E501
from .json import base64_decode, base64_decode_rows, base64_encode, base64_encode_rows  # noqa: F401
from .json import json_escape_string, json_unescape_string, json_unescape_string_rows, utf8_validate  # noqa: F401
from .json import json_index, json_index_host, json_parse_float_rows, json_parse_floats, json_print_floats  # noqa: F401
from .json import json_parse_int_rows, json_parse_ints, json_print_numbers  # noqa: F401
from .json import json_print_records  # noqa: F401
