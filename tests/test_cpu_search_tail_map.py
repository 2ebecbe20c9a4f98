"""The lane placement of k_search's sparse waves (instantavatar_amd/csrc/ia_search_tail.h) as a stand-alone host program.

The header is free of HIP types, so a C++ compiler builds it into a small program that maps 64-bit lane masks read from a
file; the properties are checked here, on its output:

  * `ia_tail_dest` is injective on the active lanes; it lands in slot 0 (lane & 3 == 0) for at most 16 survivors and in slots
    {0, 3} for at most 32; it is the identity when the mask already conforms or more than 32 lanes are active;
  * `ia_tail_src`, which the kernel pulls through, is its inverse on a wave that moves: the source of dest(l) is l, every other
    lane has none (a solve is never duplicated, never lost);
  * `ia_tail_refill_rank` numbers the idle lanes of a short pull 0 .. n - 1 in slot priority 0, 3, 1, 2, lane order inside a slot.

Masks: 10 000 random ones of EVERY population 0 .. 64, the all-ones mask, and conforming masks of both classes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(HERE, os.pardir, "instantavatar_amd", "csrc")
PER_POPULATION = 10000

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ia_search_tail.h"
// in: n uint64 masks.  out: per mask 64 bytes dest, 64 bytes src (int8, -1 = none), 64 bytes refill rank, 1 byte moves
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 3;
  uint64_t m;
  std::vector<signed char> rec(193);
  while (fread(&m, sizeof m, 1, fi) == 1) {
    for (int l = 0; l < 64; l++) {
      rec[l] = (signed char)ia_tail_dest(m, l);
      rec[64 + l] = (signed char)(ia_tail_moves(m) ? ia_tail_src(m, l) : -1);
      rec[128 + l] = (signed char)ia_tail_refill_rank(m, l);
    }
    rec[192] = (signed char)ia_tail_moves(m);
    if (fwrite(rec.data(), 1, rec.size(), fo) != rec.size()) return 4;
  }
  fclose(fo);
  return 0;
}
"""


def _compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise RuntimeError("no host C++ compiler found (c++, g++, clang++)")


def _masks(rng):
    rows = []
    for n in range(65):      # n distinct lanes out of 64: the first n of a random permutation
        perm = np.argsort(rng.rand(PER_POPULATION, 64), axis=1)[:, :n]
        rows.append((np.uint64(1) << perm.astype(np.uint64)).sum(1, dtype=np.uint64) if n else np.zeros(PER_POPULATION, np.uint64))
    slot0, slot03 = np.uint64(0x1111111111111111), np.uint64(0x9999999999999999)
    extra = [np.uint64(0xFFFFFFFFFFFFFFFF), slot0, slot03, np.uint64(0)]
    r = rng.randint(0, 2 ** 32, (2000, 2)).astype(np.uint64)
    r = r[:, 0] | (r[:, 1] << np.uint64(32))
    return np.concatenate(rows + [np.array(extra, np.uint64), r & slot0, r & slot03])     # (conforming: subsets of the slots)


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    d = tmp_path_factory.mktemp("tail_map")
    src, exe = str(d / "main.cpp"), str(d / "tail_map")
    open(src, "w").write(MAIN)
    subprocess.check_call([_compiler(), "-O1", "-std=c++17", "-Wall", "-Werror", "-I", HEADER_DIR, src, "-o", exe])
    masks = _masks(np.random.RandomState(11))
    masks.tofile(str(d / "in.bin"))
    subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
    out = np.fromfile(str(d / "out.bin"), np.int8).reshape(len(masks), 193)
    bits = ((masks[:, None] >> np.arange(64, dtype=np.uint64)[None]) & np.uint64(1)).astype(bool)
    return dict(masks=masks, act=bits, n=bits.sum(1), dest=out[:, :64].astype(np.int64), src=out[:, 64:128].astype(np.int64),
                rank=out[:, 128:192].astype(np.int64), moves=out[:, 192].astype(bool))


def _conforms(m):
    slot = np.arange(64) & 3
    in0, in03 = (slot == 0)[None], ((slot == 0) | (slot == 3))[None]
    n, act = m["n"], m["act"]
    return np.where(n <= 16, (act & ~in0).sum(1) == 0, np.where(n <= 32, (act & ~in03).sum(1) == 0, True))


def test_every_population_is_covered(mapped):
    assert (np.bincount(mapped["n"], minlength=65) >= PER_POPULATION).all()
    assert (mapped["masks"] == np.uint64(0xFFFFFFFFFFFFFFFF)).any()
    c = _conforms(mapped)
    assert (c & (mapped["n"] > 0) & (mapped["n"] <= 16)).sum() > 500 and (c & (mapped["n"] > 16) & (mapped["n"] <= 32)).sum() > 500


def test_dest_is_injective_on_the_active_lanes(mapped):
    act, dest = mapped["act"], mapped["dest"]
    assert ((dest >= 0) & (dest < 64)).all()
    row = np.broadcast_to(np.arange(len(act))[:, None], act.shape)
    hits = np.bincount((row * 64 + dest)[act], minlength=len(act) * 64)
    assert hits.max() <= 1
    assert hits.sum() == act.sum()


def test_dest_lands_in_the_slots_of_its_class(mapped):
    act, dest, n = mapped["act"], mapped["dest"], mapped["n"]
    slot = dest & 3
    small, mid = (n <= 16)[:, None] & act, ((n > 16) & (n <= 32))[:, None] & act
    assert small.any() and mid.any()
    assert (slot[small] == 0).all()
    assert np.isin(slot[mid], (0, 3)).all()


def test_identity_when_conforming_or_above_32(mapped):
    ident = (mapped["dest"] == np.arange(64)[None]).all(1)
    stay = _conforms(mapped)                       # (includes every mask of more than 32 lanes, and the empty one)
    assert np.array_equal(mapped["moves"], ~stay)
    assert ident[stay].all()
    assert (mapped["dest"] == np.arange(64)[None])[~mapped["act"]].all()        # a lane without a solve maps to itself
    assert (mapped["n"][mapped["moves"]] <= 32).all()
    # moving makes the wave conform, so it does not move again until it crosses the next threshold
    mv = np.nonzero(mapped["moves"])[0]
    after = np.zeros((len(mv), 64), bool)
    for l in range(64):
        sel = mapped["act"][mv, l]
        after[np.nonzero(sel)[0], mapped["dest"][mv[sel], l]] = True
    assert _conforms(dict(n=after.sum(1), act=after)).all() and np.array_equal(after.sum(1), mapped["n"][mv])


def test_src_is_the_inverse_of_dest(mapped):
    mv = np.nonzero(mapped["moves"])[0]
    act, dest, src = mapped["act"][mv], mapped["dest"][mv], mapped["src"][mv]
    want = np.full_like(src, -1)
    row = np.broadcast_to(np.arange(len(mv))[:, None], act.shape)
    lane = np.broadcast_to(np.arange(64)[None], act.shape)
    want[row[act], dest[act]] = lane[act]
    assert np.array_equal(src, want)
    assert (mapped["src"][~mapped["moves"]] == -1).all()


def test_refill_rank_is_the_slot_priority_order(mapped):
    need, rank = mapped["act"], mapped["rank"]            # (the same masks, read as the idle lanes of a short pull)
    prio = np.array([0, 2, 3, 1])[np.arange(64) & 3]      # slot 0 first, then 3, then 1, then 2
    key = prio * 64 + np.arange(64)
    order = np.argsort(key)                               # lanes in hand-out order
    want = np.cumsum(need[:, order], 1) - 1               # position of each idle lane in that order
    got = rank[:, order]
    assert np.array_equal(got[need[:, order]], want[need[:, order]])


def test_the_header_is_part_of_the_search_units_source_hash():
    from instantavatar_amd import build
    unit = os.path.join(build.CSRC, "ia_search.hip")
    assert os.path.join(build.CSRC, "ia_search_tail.h") in [os.path.normpath(p) for p in build.includes_of(unit)]
