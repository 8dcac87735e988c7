"""The launch planner (fastsmc_amd/csrc/fsmc_plan.h) on a CPU: tests/plan_driver.cpp, compiled here with plain g++, runs
the table below once and every field of every result is compared with the literal beside its case.

The literals were printed by the planner's text as it stood before it moved out of fsmc_capi.hip (the functions pasted
behind stub structs, fed the same table), so a difference is a change of behaviour, not of taste.  A few of them are what
the GPU tests assert on the device too (test_gpu_resident_chunks.py: 14 chunks of 48 sites, 24 rows a chunk with beta
stride 2, resident chunks = the setting)."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# WINS of test_gpu_resident_chunks.py in the driver's notation: pairs,from,to[,scan_from,scan_to]
WINS = ("64,0,640;40,3,636;64,10,331,37,300;9,100,101;33,200,202;64,300,303,301,303;64,5,422,6,421;20,0,49;"
        "64,590,640,601,640;64,0,640,100,333")

TABLE = [
    # planOneWave, member 69, the ten windows of test_gpu_resident_chunks.py
    ('planOneWave groups=WINS hard=1073741824',
     'rc=0 chunk=640 chunkRows=640 maxChunks=1 resident=0 wsSlot=743040 slots=10 waves=1 bytes=118886400 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=67108864 stride=1 resident=0',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=0 wsSlot=76032 slots=10 waves=1 bytes=12165120 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=67108864 stride=1 resident=1',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=1 wsSlot=131328 slots=10 waves=1 bytes=21012480 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=67108864 stride=1 resident=2',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=2 wsSlot=186624 slots=10 waves=1 bytes=29859840 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=1073741824 stride=1 resident=-1',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=14 wsSlot=850176 slots=10 waves=1 bytes=136028160 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=67108864 stride=2 resident=0',
     'rc=0 chunk=48 chunkRows=24 maxChunks=14 resident=0 wsSlot=48384 slots=10 waves=1 bytes=7741440 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=67108864 stride=2 resident=1',
     'rc=0 chunk=48 chunkRows=24 maxChunks=14 resident=1 wsSlot=76032 slots=10 waves=1 bytes=12165120 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=67108864 stride=2 resident=2',
     'rc=0 chunk=48 chunkRows=24 maxChunks=14 resident=2 wsSlot=103680 slots=10 waves=1 bytes=16588800 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=1073741824 stride=2 resident=-1',
     'rc=0 chunk=48 chunkRows=24 maxChunks=14 resident=14 wsSlot=435456 slots=10 waves=1 bytes=69672960 poolOff=0 poolBuffers=0 poolCap=0'),
    # the halving loop: 512 -> 64 under a limit of 100 rows; 112 (a 100-site window) -> 64 under 80 rows
    ('planOneWave groups=64,0,1000 hard=1843200',
     'rc=0 chunk=64 chunkRows=64 maxChunks=16 resident=0 wsSlot=96768 slots=1 waves=1 bytes=1548288 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=64,0,100 hard=1474560',
     'rc=0 chunk=64 chunkRows=64 maxChunks=2 resident=0 wsSlot=80640 slots=1 waves=1 bytes=1290240 poolOff=0 poolBuffers=0 poolCap=0'),
    # a limit too small; FSMC_DIAG_MAX_SLOTS below / at the group count; paired with share 2 (and alone with it)
    ('planOneWave groups=WINS hard=1048576',
     'rc=-4 why="workspace limit too small for the decode window"'),
    ('planOneWave groups=WINS hard=1073741824 maxSlots=3',
     'rc=0 chunk=640 chunkRows=640 maxChunks=1 resident=0 wsSlot=743040 slots=3 waves=1 bytes=35665920 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS hard=1073741824 maxSlots=10',
     'rc=0 chunk=640 chunkRows=640 maxChunks=1 resident=0 wsSlot=743040 slots=10 waves=1 bytes=118886400 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=1073741824 paired=1 share=2',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=0 wsSlot=76032 slots=10 waves=1 bytes=12165120 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=WINS chunkSites=48 hard=1073741824 paired=0 share=2',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=14 wsSlot=850176 slots=10 waves=1 bytes=136028160 poolOff=0 poolBuffers=0 poolCap=0'),
    # the pool: 5 groups on 2 slots (more than two rounds), 320 rows a slot; phi = 100, 200
    ('planOneWave groups=64,0,640*5 nCU=1 perCU=2 chunkSites=48 hard=11796480 phi=100',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=5 wsSlot=77184 slots=2 waves=1 bytes=11317248 poolOff=154368 poolBuffers=10 poolCap=5'),
    ('planOneWave groups=64,0,640*5 nCU=1 perCU=2 chunkSites=48 hard=11796480 phi=200',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=5 wsSlot=77184 slots=2 waves=1 bytes=11317248 poolOff=154368 poolBuffers=10 poolCap=10'),
    # not taken: chunkPool 0, exactly 2 x slots groups, sums mode, residentChunks set by the caller, no pool kernel
    ('planOneWave groups=64,0,640*5 nCU=1 perCU=2 chunkSites=48 hard=11796480 pool=0',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=5 wsSlot=352512 slots=2 waves=1 bytes=11280384 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=64,0,640*4 nCU=1 perCU=2 chunkSites=48 hard=11796480',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=5 wsSlot=352512 slots=2 waves=1 bytes=11280384 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=64,0,640*5 nCU=1 perCU=2 chunkSites=48 hard=11796480 ibd=0',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=5 wsSlot=352512 slots=2 waves=1 bytes=11280384 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=64,0,640*5 nCU=1 perCU=2 chunkSites=48 hard=11796480 resident=5',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=5 wsSlot=352512 slots=2 waves=1 bytes=11280384 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=64,0,640*5 nCU=1 perCU=2 chunkSites=48 hard=11796480 poolBuilt=0',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=5 wsSlot=352512 slots=2 waves=1 bytes=11280384 poolOff=0 poolBuffers=0 poolCap=0'),
    # chunkPool 1 with a short list; 306 rows a slot: the table row costs the last buffer (static plan: 5 chunks)
    ('planOneWave groups=64,0,640*2 nCU=1 perCU=2 chunkSites=48 hard=11796480 pool=1',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=5 wsSlot=77184 slots=2 waves=1 bytes=11317248 poolOff=154368 poolBuffers=10 poolCap=10'),
    ('planOneWave groups=64,0,640*5 nCU=1 perCU=2 chunkSites=48 hard=11280384',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=4 wsSlot=77184 slots=2 waves=1 bytes=9547776 poolOff=154368 poolBuffers=8 poolCap=8'),
    ('planOneWave groups=64,0,640*5 nCU=1 perCU=2 chunkSites=48 hard=11280384 pool=0',
     'rc=0 chunk=48 chunkRows=48 maxChunks=14 resident=5 wsSlot=352512 slots=2 waves=1 bytes=11280384 poolOff=0 poolBuffers=0 poolCap=0'),
    # wave-group members: four waves of 64 (resident chunks), eight of 80 (none); a window below the 2048 floor stays whole
    ('planOneWave groups=64,0,20000*4 member=1064 row4=64 floor=2048 poolBuilt=0 hard=2147483648',
     'rc=0 chunk=2048 chunkRows=2048 maxChunks=10 resident=2 wsSlot=25223168 slots=4 waves=1 bytes=1614282752 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=64,0,20000*4 member=8080 row4=160 floor=2048 poolBuilt=0 resBuilt=0 hard=4294967296',
     'rc=0 chunk=2048 chunkRows=2048 maxChunks=10 resident=0 wsSlot=21114880 slots=4 waves=1 bytes=1351352320 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=64,0,1500*4 member=1064 row4=64 floor=2048 poolBuilt=0 hard=2147483648 soft=1048576',
     'rc=0 chunk=1500 chunkRows=1500 maxChunks=1 resident=0 wsSlot=6164480 slots=4 waves=1 bytes=394526720 poolOff=0 poolBuffers=0 poolCap=0'),
    # workgroups per CU: the any-K kernel's four, FSMC_DIAG_WAVES_PER_CU whole, halved (two waves), not applied
    ('capWorkgroups counted=8 most=4',
     'perCU=4'),
    ('capWorkgroups counted=8 most=8 wavesPerCU=3',
     'perCU=3'),
    ('capWorkgroups counted=4 most=4 divisor=2 wavesPerCU=3',
     'perCU=1'),
    ('capWorkgroups counted=8 most=8 divisor=0 wavesPerCU=3',
     'perCU=8'),
    # any-K at K = 1100: 276 float4 a row, 11 side rows
    ('planOneWave groups=64,0,640*2000 member=0 row4=276 side=11 resBuilt=0 poolBuilt=0 perCU=4 hard=115200000000',
     'rc=0 chunk=256 chunkRows=256 maxChunks=3 resident=0 wsSlot=4769280 slots=1024 waves=1 bytes=78139883520 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planOneWave groups=64,0,30000*2000 member=0 row4=276 side=11 resBuilt=0 poolBuilt=0 perCU=4 hard=115200000000',
     'rc=0 chunk=256 chunkRows=256 maxChunks=118 resident=0 wsSlot=6800640 slots=1024 waves=1 bytes=111421685760 poolOff=0 poolBuffers=0 poolCap=0'),
    # workspaceBudget: a limit above reachable memory is cut, not below a quarter, not when memory is unknown
    ('workspaceBudget wsLimit=200000000000 memFree=100000000000',
     'hard=88480000000 soft=88480000000'),
    ('workspaceBudget wsLimit=200000000000 memFree=40000000000',
     'hard=200000000000 soft=200000000000'),
    ('workspaceBudget wsLimit=200000000000 memKnown=0',
     'hard=200000000000 soft=200000000000'),
    # no limit: memory unknown (40 %), the free allowance, a busy card; credit below / above twice the buffer; soft <= hard
    ('workspaceBudget memKnown=0 earned=400000000000',
     'hard=115200000000 soft=115200000000'),
    ('workspaceBudget memFree=280000000000',
     'hard=230400000000 soft=25769803776'),
    ('workspaceBudget memFree=100000000000',
     'hard=115200000000 soft=25769803776'),
    ('workspaceBudget earned=30000000000 cur=20000000000 wsFree=1',
     'hard=230400000000 soft=20000000000'),
    ('workspaceBudget earned=41000000000 cur=20000000000 wsFree=1',
     'hard=230400000000 soft=41000000000'),
    ('workspaceBudget earned=400000000000 cur=20000000000 wsFree=1',
     'hard=230400000000 soft=230400000000'),
    ('workspaceBudget earned=400000000000 cur=20000000000 wsFree=1 memFree=1000000000',
     'hard=115200000000 soft=115200000000'),
    # payForWorkspace; earnWorkspace
    ('payForWorkspace earned=50000000000 allocated=30000000000',
     'earned=45769803776 announced=0 announcedCredit=0'),
    ('payForWorkspace earned=50000000000 allocated=30000000000 wsFree=1',
     'earned=20000000001 announced=0 announcedCredit=0'),
    ('payForWorkspace earned=50000000000 allocated=30000000000 wsLimit=1',
     'earned=50000000000 announced=0 announcedCredit=0'),
    ('payForWorkspace earned=10 allocated=30000000000 wsFree=1',
     'earned=0 announced=0 announcedCredit=0'),
    ('earnWorkspace groups=WINS',
     'earned=17761.266035156252 announced=0 announcedCredit=0'),
    ('earnWorkspace groups=WINS ibd=0 earnScale=1000000',
     'earned=20569457285.156246 announced=0 announcedCredit=0'),
    # test_workspace_growth_is_amortised on the CPU; announce, launch, announce 0
    ('replayGrowth groups=WINS chunkSites=48 stride=2 wsFree=1',
     'rc=0 baseResident=0 baseBytes=7741440 resident=0,0,0,0,0,0,0,2,2,2,2,2,2,2,2,2,2,2,2,2,6,6,6,6 allocations=3 maxChunks=14'),
    ('announceLaunchEnd groups=WINS pairSites=1e15 wsFree=1',
     'announced: earned=288000000000 seconds=86289.0625 credit=288000000000; launched: earned=288000000000 seconds=86289.06248815915 credit=287999999960.47974; ended: earned=39.520263671875 announced=0 announcedCredit=0'),
    ('announceLaunchEnd groups=WINS pairSites=1e9 wsFree=1 earned=1000',
     'announced: earned=129434593.74999999 seconds=0.086289062499999999 credit=129433593.74999999; launched: earned=129434593.74999999 seconds=0.086277221655976566 credit=129415832.48396483; ended: earned=18761.266035154462 announced=0 announcedCredit=0'),
    # planViterbi: no states, a caller's chunk, S = 512 (hard) / 513 (soft), slots cut by the hard budget, no room
    ('planViterbi states=0',
     'rc=0 chunk=640 chunkRows=640 maxChunks=1 resident=0 wsSlot=288 slots=10 waves=1 bytes=46080 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planViterbi chunkSites=100',
     'rc=0 chunk=100 chunkRows=100 maxChunks=7 resident=0 wsSlot=36864 slots=10 waves=1 bytes=5898240 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planViterbi S=512 hard=1073741824 soft=4194304',
     'rc=0 chunk=512 chunkRows=512 maxChunks=1 resident=0 wsSlot=148608 slots=10 waves=1 bytes=23777280 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planViterbi S=513 hard=1073741824 soft=4194304',
     'rc=0 chunk=46 chunkRows=46 maxChunks=12 resident=0 wsSlot=27072 slots=10 waves=1 bytes=4331520 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planViterbi S=513 hard=1073741824 soft=4194304 nGroups=100000',
     'rc=0 chunk=46 chunkRows=46 maxChunks=12 resident=0 wsSlot=27072 slots=2048 waves=1 bytes=887095296 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planViterbi hard=1000',
     'rc=-4 why="workspace limit too small for the back-pointers of one wave"'),
    # planTwoWaves: L = 512 / 513 against soft and hard; all items resident (1024 = 256 CUs x 4; halved cap: 512)
    ('planTwoWaves groups=64,0,512*10 hard=1073741824 soft=1048576',
     'allResident=1 fits=1 rc=0 chunk=512 chunkRows=512 maxChunks=1 resident=0 wsSlot=589824 slots=10 waves=2 bytes=94371840 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planTwoWaves groups=64,0,513*10 hard=1073741824 soft=1048576',
     'allResident=1 fits=0 rc=0 chunk=513 chunkRows=513 maxChunks=1 resident=0 wsSlot=590976 slots=10 waves=2 bytes=94556160 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planTwoWaves groups=64,0,513*10 hard=1073741824',
     'allResident=1 fits=1 rc=0 chunk=513 chunkRows=513 maxChunks=1 resident=0 wsSlot=590976 slots=10 waves=2 bytes=94556160 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planTwoWaves groups=64,0,513*10 hard=1048576',
     'allResident=1 fits=0 rc=0 chunk=513 chunkRows=513 maxChunks=1 resident=0 wsSlot=590976 slots=10 waves=2 bytes=94556160 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planTwoWaves groups=64,0,512*10 nItems=1024',
     'allResident=1 fits=0 rc=0 chunk=512 chunkRows=512 maxChunks=1 resident=0 wsSlot=589824 slots=1024 waves=2 bytes=9663676416 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planTwoWaves groups=64,0,512*10 nItems=1025',
     'allResident=0 fits=0 rc=0 chunk=512 chunkRows=512 maxChunks=1 resident=0 wsSlot=589824 slots=1025 waves=2 bytes=9673113600 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planTwoWaves groups=64,0,512*10 nItems=512 wavesPerCU=4',
     'allResident=1 fits=0 rc=0 chunk=512 chunkRows=512 maxChunks=1 resident=0 wsSlot=589824 slots=512 waves=2 bytes=4831838208 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planTwoWaves groups=64,0,512*10 nItems=513 wavesPerCU=4',
     'allResident=0 fits=0 rc=0 chunk=512 chunkRows=512 maxChunks=1 resident=0 wsSlot=589824 slots=513 waves=2 bytes=4841275392 poolOff=0 poolBuffers=0 poolCap=0'),
    # staging limit, the sums' slots and stride rule
    ('staging held=0 parts=1 perItem=1000000000 nBatches=2047',
     'limit=72000000000 stagedItems=72 keepStrideOne=1'),
    ('staging wsLimit=5000000000 memFree=3000000000 held=1147483648 parts=2 perItem=300000000 nBatches=2048',
     'limit=1000000000 stagedItems=3 keepStrideOne=0'),
    ('staging memKnown=0 perItem=100000000000 sumsSlots=3',
     'limit=72000000000 stagedItems=1 keepStrideOne=1'),
    ('staging memFree=1000 perItem=176640 sumsSlots=3 perCU=0',
     'limit=0 stagedItems=1 keepStrideOne=0'),
    ('staging perItem=176640 sumsSlots=3',
     'limit=72000000000 stagedItems=3 keepStrideOne=1'),
    # slices: setting, automatic (3, all, 1 a slice), the sliceMost cap, a ragged last slice
    ('planSlices groups=WINS setting=3',
     'slice=3 nSlices=4 slicePairsMax=168 last: firstGroup=9 groups=1 firstPair=422 pairs=64'),
    ('planSlices groups=WINS setting=3 stagingBytes=100000 groupBytes=1',
     'slice=3 nSlices=4 slicePairsMax=168 last: firstGroup=9 groups=1 firstPair=422 pairs=64'),
    ('planSlices groups=WINS stagingBytes=1000 groupBytes=300',
     'slice=3 nSlices=4 slicePairsMax=168 last: firstGroup=9 groups=1 firstPair=422 pairs=64'),
    ('planSlices groups=WINS stagingBytes=1000 groupBytes=30',
     'slice=10 nSlices=1 slicePairsMax=486 last: firstGroup=0 groups=10 firstPair=0 pairs=486'),
    ('planSlices groups=WINS stagingBytes=1000 groupBytes=3000',
     'slice=1 nSlices=10 slicePairsMax=64 last: firstGroup=9 groups=1 firstPair=422 pairs=64'),
    ('planSlices groups=WINS setting=7 most=4',
     'slice=4 nSlices=3 slicePairsMax=181 last: firstGroup=8 groups=2 firstPair=358 pairs=128'),
    ('planSlices groups=WINS setting=4',
     'slice=4 nSlices=3 slicePairsMax=181 last: firstGroup=8 groups=2 firstPair=358 pairs=128'),
    # buildDualItems: inside / just outside / exactly 1.25 x; one group; lone rider, 33 pairs and a full group to rest
    ('buildDualItems groups=20,0,1000;20,200,1200',
     'dual=1 items=[0,20,0,1000,0,1000][20,20,200,1200,200,1200] unions=[0,20,0,1200,0,1200] rest='),
    ('buildDualItems groups=20,0,1000;20,251,1251',
     'dual=0'),
    ('buildDualItems groups=20,0,1000;20,250,1250',
     'dual=1 items=[0,20,0,1000,0,1000][20,20,250,1250,250,1250] unions=[0,20,0,1250,0,1250] rest='),
    ('buildDualItems groups=20,0,1000',
     'dual=0'),
    ('buildDualItems groups=20,0,1000;20,200,1200;10,5000,9000;33,0,500;64,0,3000;20,0,1000,10,900;20,100,1100,100,1000',
     'dual=1 items=[40,10,5000,9000,5000,9000][40,0,5000,9000,5000,9000][167,20,100,1100,100,1000][20,20,200,1200,200,1200][0,20,0,1000,0,1000][147,20,0,1000,10,900] unions=[40,10,5000,9000,5000,9000][167,20,100,1200,100,1200][0,20,0,1000,0,1000] rest=[50,33,0,500,0,500][83,64,0,3000,0,3000]'),
    ('buildDualItems groups=20,0,1000;64,200,1200;33,0,1000',
     'dual=0'),
    # longestFirst: ordered already; stable among equals
    ('longestFirst groups=64,0,640;64,0,640;20,0,100',
     'reordered=0 list=[0,64,0,640,0,640][64,64,0,640,0,640][128,20,0,100,0,100]'),
    ('longestFirst groups=20,0,100;64,0,640,0,600;33,5,605;64,0,640,10,600;1,0,700',
     'reordered=1 list=[181,1,0,700,0,700][20,64,0,640,0,600][84,33,5,605,5,605][117,64,0,640,10,600][0,20,0,100,0,100]'),
    # w2Member: both sides of every boundary; a valid override, one that does not hold the model tightly, one not built
    ('w2Member K=192',
     'NW=4 KH=48'),
    ('w2Member K=193',
     'NW=4 KH=64'),
    ('w2Member K=256',
     'NW=4 KH=64'),
    ('w2Member K=257',
     'NW=4 KH=80'),
    ('w2Member K=320',
     'NW=4 KH=80'),
    ('w2Member K=321',
     'NW=6 KH=64'),
    ('w2Member K=384',
     'NW=6 KH=64'),
    ('w2Member K=385',
     'NW=7 KH=64'),
    ('w2Member K=448',
     'NW=7 KH=64'),
    ('w2Member K=449',
     'NW=8 KH=64'),
    ('w2Member K=512',
     'NW=8 KH=64'),
    ('w2Member K=513',
     'NW=8 KH=80'),
    ('w2Member K=640',
     'NW=8 KH=80'),
    ('w2Member K=641',
     'NW=8 KH=96'),
    ('w2Member K=768',
     'NW=8 KH=96'),
    ('w2Member K=769',
     'NW=8 KH=128'),
    ('w2Member K=250 w2nw=4 w2kh=80',
     'NW=4 KH=80'),
    ('w2Member K=250 w2nw=7 w2kh=64',
     'NW=4 KH=64'),
    ('w2Member K=300 w2nw=5 w2kh=64',
     'NW=4 KH=80'),
    # planSamples, the other caller of planReplay, at the inputs of the planViterbi lines above (printed by the two functions
    # as they stood apart; at the table's end, so that every earlier case keeps its number):
    # the whole sequence, a caller's chunk, S = 512 (hard) / 513 (soft), slots cut by the hard budget, no room
    ('planSamples',
     'rc=0 chunk=640 chunkRows=640 maxChunks=1 resident=0 wsSlot=738432 slots=10 waves=1 bytes=118149120 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planSamples chunkSites=100',
     'rc=0 chunk=100 chunkRows=100 maxChunks=7 resident=0 wsSlot=123264 slots=10 waves=1 bytes=19722240 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planSamples S=512 hard=1073741824 soft=4194304',
     'rc=0 chunk=512 chunkRows=512 maxChunks=1 resident=0 wsSlot=590976 slots=10 waves=1 bytes=94556160 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planSamples S=513 hard=1073741824 soft=4194304',
     'rc=0 chunk=23 chunkRows=23 maxChunks=23 resident=0 wsSlot=52992 slots=10 waves=1 bytes=8478720 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planSamples S=513 hard=1073741824 soft=4194304 nGroups=100000',
     'rc=0 chunk=23 chunkRows=23 maxChunks=23 resident=0 wsSlot=52992 slots=1266 waves=1 bytes=1073405952 poolOff=0 poolBuffers=0 poolCap=0'),
    ('planSamples hard=1000',
     'rc=-4 why="workspace limit too small for the forward rows of one wave"'),
]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "fastsmc_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "plan_driver.cpp")], check=True)
    cases = "".join(case.replace("groups=WINS", "groups=" + WINS) + "\n" for case, _ in TABLE)
    out = subprocess.run([exe], input=cases, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(TABLE)
    return dict(zip((case for case, _ in TABLE), out))


def _fields(line):
    return dict(re.findall(r"(\w+)=([^ \"]+|\"[^\"]*\")", line))


@pytest.mark.parametrize("case,want", TABLE, ids=[f"{i:03d}-{c.split()[0]}" for i, (c, _) in enumerate(TABLE)])
def test_plan_table(results, case, want):
    assert results[case] == want


def test_pool_stays_inside_the_static_plans_budget(results):
    """A plan with a pool never takes more than the budget the static plan was given, and where the table row costs the
    last buffer it has one buffer less a wave."""
    for case, line in results.items():
        got = _fields(line)
        if case.startswith("planOneWave") and got.get("poolBuffers", "0") != "0":
            assert int(got["bytes"]) <= int(_fields(case)["hard"]), case
    tight = "planOneWave groups=64,0,640*5 nCU=1 perCU=2 chunkSites=48 hard=11280384"
    assert int(_fields(results[tight])["resident"]) == int(_fields(results[tight + " pool=0"])["resident"]) - 1


def test_soft_budget_never_exceeds_the_hard_one(results):
    budgets = [_fields(line) for case, line in results.items() if case.startswith("workspaceBudget")]
    assert len(budgets) >= 10 and all(int(b["soft"]) <= int(b["hard"]) for b in budgets)


def test_workspace_growth_is_amortised_on_the_cpu(results):
    """test_gpu_resident_chunks.py::test_workspace_growth_is_amortised without a device: 24 launches that each earn a third
    of the base buffer."""
    got = _fields(results["replayGrowth groups=WINS chunkSites=48 stride=2 wsFree=1"])
    resident = [int(r) for r in got["resident"].split(",")]
    assert len(resident) == 24 and got["baseResident"] == "0"
    assert resident == sorted(resident) and resident[-1] > 0
    assert resident[:4] == [0, 0, 0, 0]
    assert sum(1 for a, b in zip(resident, resident[1:]) if b != a) <= 4


def test_header_is_free_of_the_device_runtime():
    """The planner decides and does nothing: its header names no runtime call, no environment and no context."""
    text = open(os.path.join(ROOT, "fastsmc_amd", "csrc", "fsmc_plan.h")).read()
    text = text.replace('#include "../../include/fastsmc_hip.h"', "")
    for word in ("hip", "getenv", "fsmc_ctx", "fsmc_model", "chrono", "KernelFn"):
        assert word not in text.replace("chip", ""), word
