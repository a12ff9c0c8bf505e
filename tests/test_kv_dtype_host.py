"""CPU: the fp16 KV cache's C-ABI (ChattsKvCache.dtype, ChattsDecoderBuffers.kv_dtype: layout, host-side refusal of an unknown dtype)
and the kv_cache_dtype names the Python surfaces accept.  Nothing here touches a device: every call below is refused by the
argument checks before a kernel could be enqueued (the pointers are never dereferenced on the host)."""
import ctypes as C

import pytest

from chatts_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_kv_cache_struct_keeps_its_size_and_puts_dtype_in_the_hole():
    assert C.sizeof(_lib.KvCache) == 40
    assert _lib.KvCache.max_ctx.offset == 16 and _lib.KvCache.dtype.offset == 20 and _lib.KvCache.block_table.offset == 24
    assert C.sizeof(_lib.DecoderBuffers) == 176
    assert _lib.DecoderBuffers.kv_pool_blocks.offset == 168 and _lib.DecoderBuffers.kv_dtype.offset == 172
    assert _lib.KV_F32 == 0 and _lib.KV_F16 == 1
    assert _lib.KvCache(k=16, v=16, max_ctx=64).dtype == _lib.KV_F32          # zero = float32: existing callers keep their meaning


FAKE = 4096          # non-null stand-in for device pointers: the calls below must return before anything uses them


def _cache(dtype):
    return _lib.KvCache(k=FAKE, v=FAKE, max_ctx=256, dtype=dtype)


def test_unknown_kv_dtype_is_refused_by_every_cache_entry_point(lib):
    nq, nkv = 4, 2
    for dtype in (2, -1, 7):
        c = _cache(dtype)
        rc = lib.chatts_attention(FAKE, 8, nq, nkv, 0, None, C.byref(c), FAKE, 1, None, 0, None)
        assert rc == _lib.E_BADARG and b"dtype" in lib.chatts_last_error(), lib.chatts_last_error()
        rc = lib.chatts_rope_kv_write(FAKE, 8, nq, nkv, None, None, 1e-6, FAKE, FAKE, 0, None, C.byref(c), None)
        assert rc == _lib.E_BADARG and b"dtype" in lib.chatts_last_error(), lib.chatts_last_error()
        rc = lib.chatts_attention_decode_batched(FAKE, 1, nq, nkv, None, None, 1e-6, FAKE, FAKE, 5, None, C.byref(c), 0, FAKE, 4,
                                                 FAKE, 1 << 20, None)
        assert rc == _lib.E_BADARG and b"dtype" in lib.chatts_last_error(), lib.chatts_last_error()
        rc = lib.chatts_attention_decode_fused(FAKE, nq, nkv, None, None, 1e-6, FAKE, FAKE, 5, None, C.byref(c), FAKE, 4,
                                               FAKE, 1 << 20, None)
        assert rc == _lib.E_BADARG and b"dtype" in lib.chatts_last_error()


@pytest.mark.parametrize("name", [None, "auto", "float32", "fp16", "float16", "half"])
def test_kv_cache_dtype_names_accepted(name):
    from chatts_amd.modeling import kv_cache_dtype_name
    assert kv_cache_dtype_name(name) == ("float16" if name in ("fp16", "float16", "half") else "float32")


@pytest.mark.parametrize("name", ["fp8", "bf16", "bfloat16", "FP16", "", "int8", 16, ["fp16"]])
def test_kv_cache_dtype_names_rejected(name):
    from chatts_amd.modeling import kv_cache_dtype_name
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        kv_cache_dtype_name(name)
