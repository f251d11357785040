"""GPU: the device-to-host read-back entry points (gf_readback.hip), shape by shape.

Every branch a read-back can take -- plain copy below 16 MiB, the ring of eight pinned 16 MiB slots above it (whole rows per slot,
a ragged last chunk, more chunks than slots, a row wider than a slot), the direct copy into registered memory, one pipe kept open
over several blocks, the gate of a source that is still being produced, and the ring's release by gf_device_trim -- at the
smallest shape at which it can still go wrong.  The source is one seeded int64 pattern on the device; what must arrive is the
numpy slice of it, and every destination byte that no row covers must keep its sentinel."""
import ctypes as C

import numpy as np
import pytest

from golemflavor_amd import _lib, scan
from golemflavor_amd import configs as Cf
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.model import Model

pytestmark = pytest.mark.gpu

MiB = 1 << 20
SRC_BYTES = 130 * MiB                 # the largest read below (the registered gate case); every pitched block fits in it
SENTINEL = 0xA5
GATE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t)
_vp = C.c_void_p


class Readback:
    """The internal entry points bound as tools/d2h_2d_probe.py binds them, a borrowed stream, the pattern on the device."""

    def __init__(self):
        L = self.L = _lib.lib()
        L.gf_internal_borrow_stream.restype, L.gf_internal_borrow_stream.argtypes = C.c_int, [C.c_int, C.POINTER(_vp)]
        L.gf_internal_return_stream.restype, L.gf_internal_return_stream.argtypes = None, [C.c_int, _vp]
        L.gf_internal_d2h_2d.restype = C.c_int
        L.gf_internal_d2h_2d.argtypes = [C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t]
        L.gf_internal_d2h_gated.restype = C.c_int
        L.gf_internal_d2h_gated.argtypes = [C.c_int, _vp, _vp, _vp, C.c_size_t, GATE, _vp]
        L.gf_internal_d2h_pipe_open.restype, L.gf_internal_d2h_pipe_open.argtypes = C.c_int, [C.c_int, _vp, C.POINTER(_vp)]
        L.gf_internal_d2h_pipe_rows.restype = C.c_int
        L.gf_internal_d2h_pipe_rows.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t]
        L.gf_internal_d2h_pipe_close.restype, L.gf_internal_d2h_pipe_close.argtypes = C.c_int, [_vp]
        self.model = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY"))
        self.pattern = np.random.default_rng(20261017).integers(0, 2 ** 63, SRC_BYTES // 8, dtype=np.int64)
        self.bytes = self.pattern.view(np.uint8)
        self.dev = self.model.alloc(SRC_BYTES).upload(self.pattern)
        self.stream = _vp()
        assert L.gf_internal_borrow_stream(0, C.byref(self.stream)) == _lib.GF_OK
        self.arena = scan.ResultArena(SRC_BYTES + 4096)

    def close(self):
        self.arena.close()
        self.L.gf_internal_return_stream(0, self.stream)
        self.model.close()

    def want(self, off, spitch, width, height):
        """rows of the pattern: `height` rows of `width` bytes, `spitch` apart, from byte `off`"""
        return np.lib.stride_tricks.as_strided(self.bytes[off:], (height, width), (spitch, 1), writeable=False)

    def dest(self, nbytes, registered, at=0):
        """`nbytes` of sentinel: fresh pageable memory, or the arena's bytes from `at`"""
        if registered:
            assert self.arena.registered, self.arena.register_error
            d = self.arena.array.view(np.uint8)[at:at + nbytes]
            assert d.size == nbytes and np.shares_memory(d, self.arena.array)
        else:
            d = np.empty(nbytes, dtype=np.uint8)
        d[:] = SENTINEL
        return d


def check_rows(rb, dst, dpitch, off, spitch, width, height):
    """the rows arrived, and nothing between or behind them was written"""
    want = rb.want(off, spitch, width, height)
    for r in range(height):
        assert np.array_equal(dst[r * dpitch:r * dpitch + width], want[r]), "row %d" % r
        assert (dst[r * dpitch + width:(r + 1) * dpitch] == SENTINEL).all(), "behind row %d" % r


@pytest.fixture(scope="module")
def rb():
    r = Readback()
    yield r
    r.close()


# width (spitch = width + 4096, dpitch = width + 24), height: see the module docstring
PITCHED = {
    "below_the_threshold": (1 * MiB + 8, 3),
    "five_rows_per_slot_ragged_last_chunk": (3 * MiB + 8, 6),
    "one_row_per_slot_ring_wraps": (9 * MiB + 8, 10),
    "row_wider_than_a_slot": (16 * MiB + 8, 2),
}


@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "arena"])
@pytest.mark.parametrize("shape", list(PITCHED))
def test_pitched_copy(rb, shape, registered):
    width, height = PITCHED[shape]
    spitch, dpitch = width + 4096, width + 24
    dst = rb.dest(height * dpitch, registered)
    rc = rb.L.gf_internal_d2h_2d(0, rb.stream, dst.ctypes.data, dpitch, rb.dev.at(8), spitch, width, height)
    assert rc == _lib.GF_OK, rb.L.gf_last_hip_error()
    check_rows(rb, dst, dpitch, 8, spitch, width, height)


@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "arena"])
def test_packed_rows_take_the_linear_route(rb, registered):
    width, height = 4 * MiB, 5                                  # width == dpitch == spitch, 20 MiB in all
    dst = rb.dest(width * height + 64, registered)
    rc = rb.L.gf_internal_d2h_2d(0, rb.stream, dst.ctypes.data, width, rb.dev.at(16), width, width, height)
    assert rc == _lib.GF_OK, rb.L.gf_last_hip_error()
    assert np.array_equal(dst[:width * height], rb.bytes[16:16 + width * height])
    assert (dst[width * height:] == SENTINEL).all()


def test_an_empty_block_writes_nothing(rb):
    dst = rb.dest(4096, False)
    for width, height in ((0, 3), (1024, 0), (0, 0)):
        assert rb.L.gf_internal_d2h_2d(0, rb.stream, dst.ctypes.data, 1024, rb.dev.at(0), 2048, width, height) == _lib.GF_OK
    assert (dst == SENTINEL).all()


@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "arena"])
def test_one_pipe_over_several_blocks(rb, registered):
    """a block below the synchronous entry points' threshold (through the ring all the same: a pipe has none), whole rows per slot
    in two chunks, rows wider than a slot; checked after the close, the only point at which a pipe's destinations are final"""
    blocks, at = [], 0                                          # (source offset, width, height), one destination each
    for off, width, height in ((0, 512 * 1024, 4), (24, 2 * MiB + 8, 9), (40, 16 * MiB + 8, 2)):
        spitch, dpitch = width + 4096, width + 24
        dst = rb.dest(height * dpitch, registered, at)
        at += (height * dpitch + 4095) // 4096 * 4096
        blocks.append((dst, dpitch, off, spitch, width, height))
    p = _vp()
    assert rb.L.gf_internal_d2h_pipe_open(0, rb.stream, C.byref(p)) == _lib.GF_OK and p
    for dst, dpitch, off, spitch, width, height in blocks:
        rc = rb.L.gf_internal_d2h_pipe_rows(p, dst.ctypes.data, dpitch, rb.dev.at(off), spitch, width, height)
        assert rc == _lib.GF_OK, rb.L.gf_last_hip_error()
    assert rb.L.gf_internal_d2h_pipe_close(p) == _lib.GF_OK, rb.L.gf_last_hip_error()
    for dst, dpitch, off, spitch, width, height in blocks:
        check_rows(rb, dst, dpitch, off, spitch, width, height)


def test_a_pipe_without_rows_closes_clean(rb):
    p = _vp()
    assert rb.L.gf_internal_d2h_pipe_open(0, rb.stream, C.byref(p)) == _lib.GF_OK and p
    assert rb.L.gf_internal_d2h_pipe_close(p) == _lib.GF_OK
    assert rb.L.gf_internal_d2h_pipe_close(None) == _lib.GF_OK


@pytest.mark.parametrize("case,registered,nbytes,calls", [
    ("ring_16MiB_chunks", False, 40 * MiB + 8, [16 * MiB, 32 * MiB, 40 * MiB + 8]),
    ("direct_64MiB_pieces", True, 130 * MiB, [64 * MiB, 128 * MiB, 130 * MiB]),
    ("plain_copy_one_call", False, 1 * MiB, [1 * MiB]),
])
def test_the_gate_is_asked_before_every_piece(rb, case, registered, nbytes, calls):
    """gate(ctx, upto) precedes each piece with the end offset of that piece: 16 MiB ring chunks into pageable memory, 64 MiB pieces
    into registered memory, one call for a copy below the ring's threshold"""
    seen = []
    gate = GATE(lambda ctx, upto: seen.append(upto) or 0)
    dst = rb.dest(nbytes + 64, registered)
    rc = rb.L.gf_internal_d2h_gated(0, rb.stream, dst.ctypes.data, rb.dev.at(0), nbytes, gate, None)
    assert rc == _lib.GF_OK, rb.L.gf_last_hip_error()
    assert seen == calls
    assert np.array_equal(dst[:nbytes], rb.bytes[:nbytes]) and (dst[nbytes:] == SENTINEL).all()


def test_a_refusing_gate_ends_the_copy(rb):
    """a host-side return code: the gate says the source was not completed, the call returns GF_ERR_HIP without asking again, the
    consumer thread is joined, and the ring serves the next read"""
    seen = []
    gate = GATE(lambda ctx, upto: seen.append(upto) or (1 if len(seen) == 2 else 0))
    nbytes = 40 * MiB + 8
    dst = rb.dest(nbytes, False)
    rc = rb.L.gf_internal_d2h_gated(0, rb.stream, dst.ctypes.data, rb.dev.at(0), nbytes, gate, None)
    assert rc == _lib.GF_ERR_HIP
    assert b"completed" in rb.L.gf_last_hip_error()
    assert seen == [16 * MiB, 32 * MiB]
    assert np.array_equal(dst[:16 * MiB], rb.bytes[:16 * MiB])  # the piece issued before the refusal has arrived: no copy is left in flight
    assert (dst[16 * MiB:] == SENTINEL).all()                   # nothing of the refused piece or behind it
    back = rb.dest(20 * MiB, False)
    _lib.check(rb.L.gf_memcpy_d2h(rb.model._h, back.ctypes.data, rb.dev.at(32 * MiB), back.size), "d2h")
    assert np.array_equal(back, rb.bytes[32 * MiB:32 * MiB + back.size])


def test_trim_releases_the_ring_and_the_next_read_allocates_it_again(rb):
    for _ in range(2):
        back = rb.dest(20 * MiB, False)
        _lib.check(rb.L.gf_memcpy_d2h(rb.model._h, back.ctypes.data, rb.dev.at(64), back.size), "d2h")
        assert np.array_equal(back, rb.bytes[64:64 + back.size])
        _lib.device_trim(0)
