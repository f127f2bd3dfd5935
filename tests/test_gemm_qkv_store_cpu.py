"""The LDS maps of gemm_epilogue_wreg_qkv_lds (csrc/gemm_f16.h: qkv_lds_off, qkv_lds_park, qkv_lds_read), evaluated on the host through the harness library: the
kernel computes its addresses with these very constexpr functions.

A wave pair owns one 16 KB image of its 64-column half of the tile. For the Q / K form and the V form: the pieces the two waves park (8 bytes per lane and
accumulator) tile the image exactly once, so do the pieces they read back (16 bytes per lane and pass), each piece is contiguous in the image, the read-out meets
every element the parking put there, and no group of lanes that the LDS serves together meets a bank twice: 64 banks of 4 bytes; an 8-byte write is served 32
lanes at a time, a 16-byte read 16 lanes at a time."""
import ctypes as C

import pytest

import gemm_cases as G

IMG = 16384


@pytest.fixture(scope="module")
def maps():
    L = G.harness()
    f = L.tts_gemm_test_qkv_lds
    f.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)] * 2
    f.restype = C.c_int

    def call(read, nat, wave, lane, a, b=0):
        r, c = C.c_int(), C.c_int()
        off = f(read, nat, wave, lane, a, b, C.byref(r), C.byref(c))
        return off, r.value, c.value
    return call


def _banks(off, nbytes):
    return {(off + d) // 4 % 64 for d in range(0, nbytes, 4)}


@pytest.mark.parametrize("nat", (0, 1), ids=("qk", "v"))
def test_parking_and_read_out(maps, nat):
    parked, where = {}, {}  # byte offset -> piece; element (r, c) -> byte offset
    for wave in (0, 1):
        for i in range(8):
            for j in range(2):
                offs = [maps(0, nat, wave, lane, i, j) for lane in range(64)]
                for lane, (off, r, c) in enumerate(offs):
                    assert off % 8 == 0 and 0 <= off <= IMG - 8 and off not in parked, (wave, lane, i, j, off)
                    parked[off] = (r, c)
                    fr, fq = lane & 15, lane >> 4  # the accumulator layout the epilogue states: swapped order rows fr, columns 4 fq ..; natural order the transpose
                    want = (32 * wave + 16 * j + fr, 16 * i + 4 * fq) if nat else (16 * i + fr, 32 * wave + 16 * j + 4 * fq)
                    assert (r, c) == want, (wave, lane, i, j)
                    for e in range(4):
                        where[(r, c + e)] = off + 2 * e
                for g0 in (0, 32):
                    banks = [b for off, _, _ in offs[g0:g0 + 32] for b in _banks(off, 8)]
                    assert len(set(banks)) == 64, ("parking", wave, i, j, g0)
    assert len(parked) == IMG // 8 and len(where) == IMG // 2
    dims = (64, 128) if nat else (128, 64)
    assert set(where) == {(r, c) for r in range(dims[0]) for c in range(dims[1])}
    read = set()
    for wave in (0, 1):
        for p in range(8):
            offs = [maps(1, nat, wave, lane, p) for lane in range(64)]
            for lane, (off, r, c) in enumerate(offs):
                assert off % 16 == 0 and off not in read, (wave, lane, p, off)
                read.add(off)
                assert [where[(r, c + e)] for e in range(8)] == [off + 2 * e for e in range(8)], (wave, lane, p)  # 8 consecutive elements = 16 contiguous bytes
                # 16 (Q / K: 8) adjacent lanes store one contiguous run of a channel's (a row's) output line
                per = 16 if nat else 8
                assert (r, c) == (offs[lane - lane % per][1], 8 * (lane % per)), (wave, lane, p)
            for g0 in range(0, 64, 16):
                banks = [b for off, _, _ in offs[g0:g0 + 16] for b in _banks(off, 16)]
                assert len(set(banks)) == 64, ("read-out", wave, p, g0)
    assert len(read) == IMG // 16
