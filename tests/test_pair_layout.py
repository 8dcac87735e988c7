"""The device buffers of the seven fsmc_decode_pair_* entry points (fastsmc_amd/csrc/fsmc_pair_layout.h) on a CPU:
tests/pair_layout_driver.cpp, compiled here with plain g++, runs the table below once and every field of every layout is
compared with the literal beside its case.

The literals were printed by the entry points' own expressions as they stood in fsmc_capi.hip before the layouts moved
out of it -- the size each passed to its allocation, the offsets it then recomputed for its kernels and the bytes a group
it stated to the slice planner, pasted into a scratch program and fed the same table -- so a difference is a change of
behaviour.  The invariants below are checked by this file from the printed regions (name=offset:bytes:element size), on
every case: they hold for the layouts as they were; the numbers are the parent's either way."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = [
    ('posteriors K=69 S=1 slice=1 pairs=1 rows=1',
     'groupBytes=35328 stageBytes=17664 rowBytes=276 rowsBytes=276 accBytes=552 coal=0:276:4 sum=276:276:4'),
    ('posteriors K=69 S=1 slice=1 pairs=1 rows=0',
     'groupBytes=17664 stageBytes=17664 rowBytes=276 rowsBytes=0 accBytes=552 coal=0:276:4 sum=276:276:4'),
    ('posteriors K=5 S=65 slice=2 pairs=70 rows=1',
     'groupBytes=166400 stageBytes=166400 rowBytes=1300 rowsBytes=91000 accBytes=1320 coal=0:20:4 sum=20:1300:4'),
    ('posteriors K=5 S=65 slice=2 pairs=70 rows=0',
     'groupBytes=83200 stageBytes=166400 rowBytes=1300 rowsBytes=0 accBytes=1320 coal=0:20:4 sum=20:1300:4'),
    ('posteriors K=69 S=640 slice=10 pairs=486 rows=1',
     'groupBytes=22609920 stageBytes=113049600 rowBytes=176640 rowsBytes=85847040 accBytes=176916 coal=0:276:4 sum=276:176640:4'),
    ('posteriors K=69 S=6760 slice=64 pairs=4096 rows=1',
     'groupBytes=238817280 stageBytes=7642152960 rowBytes=1865760 rowsBytes=7642152960 accBytes=1866036 coal=0:276:4 sum=276:1865760:4'),
    ('minima KP=80 S=1 pairs=1 nOut=1',
     'groupBytes=256 siteBlocks=1 rangeLen=16 rangesMax=1 tooManyRanges=0 stageBytes=4 vec=4 accBytes=352 coal=0:320:4 minMean=320:4:4 argMean=324:4:4 minMap=328:4:4 argMap=332:4:4 part.minMean=336:4:4 part.argMean=340:4:4 part.minMap=344:4:4 part.argMap=348:4:4'),
    ('minima KP=80 S=1 pairs=1 nOut=2',
     'groupBytes=512 siteBlocks=1 rangeLen=16 rangesMax=1 tooManyRanges=0 stageBytes=8 vec=4 accBytes=352 coal=0:320:4 minMean=320:4:4 argMean=324:4:4 minMap=328:4:4 argMap=332:4:4 part.minMean=336:4:4 part.argMean=340:4:4 part.minMap=344:4:4 part.argMap=348:4:4'),
    ('minima KP=16 S=65 pairs=70 nOut=2',
     'groupBytes=33280 siteBlocks=2 rangeLen=16 rangesMax=5 tooManyRanges=0 stageBytes=36400 vec=260 accBytes=6304 coal=0:64:4 minMean=64:260:4 argMean=324:260:4 minMap=584:260:4 argMap=844:260:4 part.minMean=1104:1300:4 part.argMean=2404:1300:4 part.minMap=3704:1300:4 part.argMap=5004:1300:4'),
    ('minima KP=16 S=65 pairs=70 nOut=1 minimaRange=7',
     'groupBytes=16640 siteBlocks=2 rangeLen=7 rangesMax=10 tooManyRanges=0 stageBytes=18200 vec=260 accBytes=11504 coal=0:64:4 minMean=64:260:4 argMean=324:260:4 minMap=584:260:4 argMap=844:260:4 part.minMean=1104:2600:4 part.argMean=3704:2600:4 part.minMap=6304:2600:4 part.argMap=8904:2600:4'),
    ('minima KP=16 S=65 pairs=70 nOut=2 minimaRange=1',
     'groupBytes=33280 siteBlocks=2 rangeLen=1 rangesMax=70 tooManyRanges=0 stageBytes=36400 vec=260 accBytes=73904 coal=0:64:4 minMean=64:260:4 argMean=324:260:4 minMap=584:260:4 argMap=844:260:4 part.minMean=1104:18200:4 part.argMean=19304:18200:4 part.minMap=37504:18200:4 part.argMap=55704:18200:4'),
    ('minima KP=80 S=640 pairs=486 nOut=2 minimaRange=16',
     'groupBytes=327680 siteBlocks=10 rangeLen=16 rangesMax=31 tooManyRanges=0 stageBytes=2488320 vec=2560 accBytes=328000 coal=0:320:4 minMean=320:2560:4 argMean=2880:2560:4 minMap=5440:2560:4 argMap=8000:2560:4 part.minMean=10560:79360:4 part.argMean=89920:79360:4 part.minMap=169280:79360:4 part.argMap=248640:79360:4'),
    ('minima KP=80 S=640 pairs=486 nOut=2 minimaRange=100',
     'groupBytes=327680 siteBlocks=10 rangeLen=16 rangesMax=31 tooManyRanges=0 stageBytes=2488320 vec=2560 accBytes=328000 coal=0:320:4 minMean=320:2560:4 argMean=2880:2560:4 minMap=5440:2560:4 argMap=8000:2560:4 part.minMean=10560:79360:4 part.argMean=89920:79360:4 part.minMap=169280:79360:4 part.argMap=248640:79360:4'),
    ('minima KP=80 S=6760 pairs=499500 nOut=2',
     'groupBytes=3461120 siteBlocks=106 rangeLen=12808 rangesMax=39 tooManyRanges=0 stageBytes=27012960000 vec=27040 accBytes=4326720 coal=0:320:4 minMean=320:27040:4 argMean=27360:27040:4 minMap=54400:27040:4 argMap=81440:27040:4 part.minMean=108480:1054560:4 part.argMean=1163040:1054560:4 part.minMap=2217600:1054560:4 part.argMap=3272160:1054560:4'),
    ('minima KP=80 S=6760 pairs=499500 nOut=2 nCU=1',
     'groupBytes=3461120 siteBlocks=106 rangeLen=499500 rangesMax=1 tooManyRanges=0 stageBytes=27012960000 vec=27040 accBytes=216640 coal=0:320:4 minMean=320:27040:4 argMean=27360:27040:4 minMap=54400:27040:4 argMap=81440:27040:4 part.minMean=108480:27040:4 part.argMean=135520:27040:4 part.minMap=162560:27040:4 part.argMap=189600:27040:4'),
    ('minima KP=80 S=50000 pairs=4000000 nOut=2 minimaRange=1',
     'groupBytes=25600000 siteBlocks=782 rangeLen=1 rangesMax=4000000 tooManyRanges=1 stageBytes=1600000000000 vec=200000 accBytes=3200000800320 coal=0:320:4 minMean=320:200000:4 argMean=200320:200000:4 minMap=400320:200000:4 argMap=600320:200000:4 part.minMean=800320:800000000000:4 part.argMean=800000800320:800000000000:4 part.minMap=1600000800320:800000000000:4 part.argMap=2400000800320:800000000000:4'),
    ('minima KP=80 S=50000 pairs=2000000 nOut=2 minimaRange=1',
     'groupBytes=25600000 siteBlocks=782 rangeLen=1 rangesMax=2000000 tooManyRanges=0 stageBytes=800000000000 vec=200000 accBytes=1600000800320 coal=0:320:4 minMean=320:200000:4 argMean=200320:200000:4 minMap=400320:200000:4 argMap=600320:200000:4 part.minMean=800320:400000000000:4 part.argMean=400000800320:400000000000:4 part.minMap=800000800320:400000000000:4 part.argMap=1200000800320:400000000000:4'),
    ('bins KP=80 S=1 B=1 pairs=1 nRows=2',
     'groupBytes=1792 stageBytes=8 edgeBytes=8 outBytes=4 accBytes=348 coal=0:320:4 edges=320:8:4 mean=328:4:4 minMean=332:4:4 argMean=336:4:4 minMap=340:4:4 argMap=344:4:4'),
    ('bins KP=80 S=1 B=1 pairs=1 nRows=1 minMap=0 argMap=0',
     'groupBytes=1024 stageBytes=4 edgeBytes=8 outBytes=4 accBytes=340 coal=0:320:4 edges=320:8:4 mean=328:4:4 minMean=332:4:4 argMean=336:4:4'),
    ('bins KP=80 S=1 B=1 pairs=1 nRows=1 mean=0 minMean=0 argMean=0',
     'groupBytes=768 stageBytes=4 edgeBytes=8 outBytes=4 accBytes=336 coal=0:320:4 edges=320:8:4 minMap=328:4:4 argMap=332:4:4'),
    ('bins KP=16 S=65 B=3 pairs=70 nRows=2',
     'groupBytes=37120 stageBytes=36400 edgeBytes=16 outBytes=840 accBytes=4280 coal=0:64:4 edges=64:16:4 mean=80:840:4 minMean=920:840:4 argMean=1760:840:4 minMap=2600:840:4 argMap=3440:840:4'),
    ('bins KP=16 S=65 B=3 pairs=70 nRows=1 mean=0 minMap=0 argMap=0',
     'groupBytes=18176 stageBytes=18200 edgeBytes=16 outBytes=840 accBytes=1760 coal=0:64:4 edges=64:16:4 minMean=80:840:4 argMean=920:840:4'),
    ('bins KP=16 S=65 B=3 pairs=70 nRows=2 minMean=0 argMean=0',
     'groupBytes=35584 stageBytes=36400 edgeBytes=16 outBytes=840 accBytes=2600 coal=0:64:4 edges=64:16:4 mean=80:840:4 minMap=920:840:4 argMap=1760:840:4'),
    ('bins KP=16 S=65 B=3 pairs=70 nRows=1 minMean=0 argMean=0 minMap=0 argMap=0',
     'groupBytes=17408 stageBytes=18200 edgeBytes=16 outBytes=840 accBytes=920 coal=0:64:4 edges=64:16:4 mean=80:840:4'),
    ('bins KP=80 S=640 B=64 pairs=486 nRows=2 mean=0',
     'groupBytes=393216 stageBytes=2488320 edgeBytes=260 outBytes=124416 accBytes=498244 coal=0:320:4 edges=320:260:4 minMean=580:124416:4 argMean=124996:124416:4 minMap=249412:124416:4 argMap=373828:124416:4'),
    ('loglik B=0 pairs=1',
     'groupBytes=768 edgeBytes=4 accBytes=16 mant=0:8:8 binMant=8:0:8 expo=8:4:4 binExpo=12:0:4 edges=12:4:4'),
    ('loglik B=1 pairs=1',
     'groupBytes=1536 edgeBytes=8 accBytes=32 mant=0:8:8 binMant=8:8:8 expo=16:4:4 binExpo=20:4:4 edges=24:8:4'),
    ('loglik B=3 pairs=70',
     'groupBytes=3072 edgeBytes=16 accBytes=3376 mant=0:560:8 binMant=560:1680:8 expo=2240:280:4 binExpo=2520:840:4 edges=3360:16:4'),
    ('loglik B=0 pairs=70',
     'groupBytes=768 edgeBytes=4 accBytes=844 mant=0:560:8 binMant=560:0:8 expo=560:280:4 binExpo=840:0:4 edges=840:4:4'),
    ('loglik B=3 pairs=3',
     'groupBytes=3072 edgeBytes=16 accBytes=160 mant=0:24:8 binMant=24:72:8 expo=96:12:4 binExpo=108:36:4 edges=144:16:4'),
    ('loglik B=64 pairs=4096',
     'groupBytes=49920 edgeBytes=260 accBytes=3195140 mant=0:32768:8 binMant=32768:2097152:8 expo=2129920:16384:4 binExpo=2146304:1048576:4 edges=3194880:260:4'),
    ('viterbi S=1 pairs=1',
     'groupBytes=832 rowsBytes=4 accBytes=12 mant=0:8:8 expo=8:4:4'),
    ('viterbi S=1 pairs=1 states=0',
     'groupBytes=768 rowsBytes=4 accBytes=12 mant=0:8:8 expo=8:4:4'),
    ('viterbi S=1 pairs=1 prob=0',
     'groupBytes=64 rowsBytes=4 accBytes=12 mant=0:8:8 expo=8:4:4'),
    ('viterbi S=65 pairs=70',
     'groupBytes=4928 rowsBytes=4552 accBytes=840 mant=0:560:8 expo=560:280:4'),
    ('viterbi S=65 pairs=3 prob=0',
     'groupBytes=4160 rowsBytes=196 accBytes=36 mant=0:24:8 expo=24:12:4'),
    ('viterbi S=65 pairs=70 states=0',
     'groupBytes=768 rowsBytes=4552 accBytes=840 mant=0:560:8 expo=560:280:4'),
    ('viterbi S=640 pairs=486',
     'groupBytes=41728 rowsBytes=311040 accBytes=5832 mant=0:3888:8 expo=3888:1944:4'),
    ('cdf K=69 S=1 nOut=1 slice=1 pairs=1',
     'groupBytes=17920 sliceMost=2147483647 stageBytes=17664 outCells=1 rowsBytes=4 specBytes=8'),
    ('cdf K=5 S=65 nOut=3 slice=2 pairs=70',
     'groupBytes=133120 sliceMost=1073741823 stageBytes=166400 outCells=4550 rowsBytes=54600 specBytes=24'),
    ('cdf K=69 S=65 nOut=16 slice=2 pairs=70',
     'groupBytes=1414400 sliceMost=1073741823 stageBytes=2296320 outCells=4550 rowsBytes=291200 specBytes=128'),
    ('cdf K=69 S=640 nOut=4 slice=10 pairs=486',
     'groupBytes=11960320 sliceMost=214748364 stageBytes=113049600 outCells=311040 rowsBytes=4976640 specBytes=32'),
    ('cdf K=5 S=64 nOut=1 slice=1 pairs=64',
     'groupBytes=98304 sliceMost=2147483647 stageBytes=81920 outCells=4096 rowsBytes=16384 specBytes=8'),
    ('tail K=69 S=1 nTail=1 slice=1 pairs=1',
     'groupBytes=17920 sliceMost=2147483647 stageBytes=17664 rowsBytes=4 specBytes=8 sumBytes=8 outBytes=0 accBytes=8 sum=0:8:8'),
    ('tail K=69 S=1 nTail=1 B=1 slice=1 pairs=1 mean=1',
     'groupBytes=18176 sliceMost=2147483647 stageBytes=17664 rowsBytes=4 specBytes=8 sumBytes=8 outBytes=4 accBytes=20 sum=0:8:8 edges=8:8:4 binMean=16:4:4'),
    ('tail K=69 S=1 nTail=1 B=1 slice=1 pairs=1 length=1',
     'groupBytes=18176 sliceMost=2147483647 stageBytes=17664 rowsBytes=4 specBytes=8 sumBytes=8 outBytes=4 accBytes=28 sum=0:8:8 edges=8:8:4 weights=16:4:4 binLength=24:4:4'),
    ('tail K=69 S=1 nTail=1 B=1 slice=1 pairs=1 mean=1 length=1',
     'groupBytes=18432 sliceMost=2147483647 stageBytes=17664 rowsBytes=4 specBytes=8 sumBytes=8 outBytes=4 accBytes=32 sum=0:8:8 edges=8:8:4 weights=16:4:4 binMean=24:4:4 binLength=28:4:4'),
    ('tail K=5 S=65 nTail=3 slice=2 pairs=70',
     'groupBytes=133120 sliceMost=1073741823 stageBytes=166400 rowsBytes=54600 specBytes=24 sumBytes=1560 outBytes=0 accBytes=1560 sum=0:1560:8'),
    ('tail K=5 S=65 nTail=3 B=3 slice=2 pairs=70 mean=1',
     'groupBytes=135424 sliceMost=1073741823 stageBytes=166400 rowsBytes=54600 specBytes=24 sumBytes=1560 outBytes=2520 accBytes=4096 sum=0:1560:8 edges=1560:16:4 binMean=1576:2520:4'),
    ('tail K=5 S=65 nTail=3 B=3 slice=2 pairs=70 length=1',
     'groupBytes=135424 sliceMost=1073741823 stageBytes=166400 rowsBytes=54600 specBytes=24 sumBytes=1560 outBytes=2520 accBytes=4360 sum=0:1560:8 edges=1560:16:4 weights=1576:260:4 binLength=1840:2520:4'),
    ('tail K=5 S=65 nTail=3 B=3 slice=2 pairs=70 mean=1 length=1',
     'groupBytes=137728 sliceMost=1073741823 stageBytes=166400 rowsBytes=54600 specBytes=24 sumBytes=1560 outBytes=2520 accBytes=6880 sum=0:1560:8 edges=1560:16:4 weights=1576:260:4 binMean=1840:2520:4 binLength=4360:2520:4'),
    ('tail K=69 S=65 nTail=3 B=2 slice=2 pairs=70 mean=1 length=1',
     'groupBytes=1201152 sliceMost=1073741823 stageBytes=2296320 rowsBytes=54600 specBytes=24 sumBytes=1560 outBytes=1680 accBytes=5200 sum=0:1560:8 edges=1560:12:4 weights=1576:260:4 binMean=1840:1680:4 binLength=3520:1680:4'),
    ('tail K=69 S=640 nTail=8 B=64 slice=10 pairs=486 mean=1 length=1',
     'groupBytes=12877824 sliceMost=214748364 stageBytes=113049600 rowsBytes=9953280 specBytes=64 sumBytes=40960 outBytes=995328 accBytes=2034440 sum=0:40960:8 edges=40960:260:4 weights=41224:2560:4 binMean=43784:995328:4 binLength=1039112:995328:4'),
]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_layout") / "pair_layout_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "fastsmc_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "pair_layout_driver.cpp")], check=True)
    cases = "".join(case + "\n" for case, _ in TABLE)
    out = subprocess.run([exe], input=cases, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(TABLE)
    return dict(zip((case for case, _ in TABLE), out))


def _fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)(?= |$)", line)}


def _regions(line):
    """(name, offset, bytes, element size) of the accumulator's regions, in the order they were printed."""
    return [(n, int(o), int(b), int(e)) for n, o, b, e in re.findall(r"([\w.]+)=(\d+):(\d+):(\d+)", line)]


@pytest.mark.parametrize("case,want", TABLE, ids=[f"{i:02d}-{c.split()[0]}" for i, (c, _) in enumerate(TABLE)])
def test_layout_table(results, case, want):
    assert results[case] == want


def test_every_entry_point_has_its_cases():
    for name in ("posteriors", "minima", "bins", "loglik", "viterbi", "cdf", "tail"):
        assert sum(1 for case, _ in TABLE if case.split()[0] == name) >= 5, name


@pytest.mark.parametrize("case", [c for c, _ in TABLE], ids=[f"{i:02d}-{c.split()[0]}" for i, (c, _) in enumerate(TABLE)])
def test_regions_are_disjoint_ordered_aligned_and_fill_the_buffer(results, case):
    line = results[case]
    regions = _regions(line)
    if case.split()[0] == "cdf":
        assert regions == []  # (no accumulator: its outputs are ppRows, [output][pair][S])
        return
    assert regions and regions[0][1] == 0
    end = 0
    for name, off, size, elem in regions:
        assert size >= 0 and off >= 0, name  # (read as unsigned: a negative size would show as an offset out of order)
        assert off >= end, (name, off, end)  # ascending and disjoint
        assert off % elem == 0, (name, off, elem)  # 8 for the double regions
        end = off + size
    assert _fields(line)["accBytes"] == end  # the total is the end of the last region
    assert end < 1 << 62


def test_minima_ranges(results):
    seen_overflow = set()
    for case, line in results.items():
        if not case.startswith("minima"):
            continue
        got, given = _fields(line), _fields(case)
        if "minimaRange" not in given:
            assert got["rangeLen"] >= 16, case
        else:  # the diagnostic value lowers the range, never raises it, and a range has a pair at least
            assert 1 <= got["rangeLen"] <= max(16, given["minimaRange"]), case
        assert got["rangesMax"] * got["rangeLen"] >= given["pairs"], case
        assert (got["rangesMax"] - 1) * got["rangeLen"] < given["pairs"], case
        assert got["siteBlocks"] == (given["S"] + 63) // 64
        # the overflow condition, as the entry point had it: ranges x site blocks beyond INT32_MAX
        assert got["tooManyRanges"] == (1 if got["rangesMax"] * got["siteBlocks"] > 2 ** 31 - 1 else 0), case
        seen_overflow.add(got["tooManyRanges"])
    assert seen_overflow == {0, 1}


def test_group_bytes_cover_a_full_groups_share_of_the_buffers(results):
    """What the slice planner divides the staging limit by is no less than what a full group of 64 pairs takes of the
    buffers sized by the slice (the accumulators' fixed parts -- coalescence times, edges, carried sums -- aside)."""
    for case, line in results.items():
        got, given = _fields(line), _fields(case)
        name = case.split()[0]
        if name in ("posteriors", "cdf", "tail") and given["pairs"] <= 64 * given["slice"]:
            assert got["stageBytes"] + got["rowsBytes"] <= given["slice"] * got["groupBytes"], case


def test_header_is_free_of_the_device_runtime():
    """The layouts decide and do nothing: the header names no runtime call, no environment and no context."""
    text = open(os.path.join(ROOT, "fastsmc_amd", "csrc", "fsmc_pair_layout.h")).read()
    for word in ("hip", "getenv", "fsmc_ctx", "fsmc_model", "chrono", "KernelFn"):
        assert word not in text.replace("chip", ""), word
