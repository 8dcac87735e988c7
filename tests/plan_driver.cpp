// plan_driver.cpp -- fsmc_plan.h on a CPU: reads cases from stdin, one a line, and prints every field of each result on
// one line (tests/test_plan.py holds the table and the expected lines).
//
// A case is a function's name and key=value inputs; a key left out has the default below.  Work lists:
// groups=<pairs>,<from>,<to>[,<scan_from>,<scan_to>][*<times>];...  (first_pair counts up; the scan window is the window
// where it is left out).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "fsmc_plan.h"

using namespace fsmc::plan;

namespace
{
struct Case {
  std::map<std::string, std::string> kv;
  uint64_t u(const char* key, uint64_t dflt) const
  {
    const auto it = kv.find(key);
    return it == kv.end() ? dflt : std::strtoull(it->second.c_str(), nullptr, 10);
  }
  long i(const char* key, long dflt) const
  {
    const auto it = kv.find(key);
    return it == kv.end() ? dflt : std::atol(it->second.c_str());
  }
  double d(const char* key, double dflt) const
  {
    const auto it = kv.find(key);
    return it == kv.end() ? dflt : std::atof(it->second.c_str());
  }
  std::vector<fsmc_group> groups() const
  {
    std::vector<fsmc_group> out;
    const auto it = kv.find("groups");
    if (it == kv.end()) {
      return out;
    }
    std::stringstream all(it->second);
    std::string one;
    uint32_t first = 0;
    while (std::getline(all, one, ';')) {
      unsigned long v[5] = {0, 0, 0, 0, 0}, times = 1;
      const size_t star = one.find('*');
      if (star != std::string::npos) {
        times = std::strtoul(one.c_str() + star + 1, nullptr, 10);
        one.resize(star);
      }
      const int n = std::sscanf(one.c_str(), "%lu,%lu,%lu,%lu,%lu", &v[0], &v[1], &v[2], &v[3], &v[4]);
      for (unsigned long t = 0; t < times; ++t) {
        fsmc_group g;
        g.first_pair = first;
        g.n_pairs = (uint32_t)v[0];
        g.from = (uint32_t)v[1];
        g.to = (uint32_t)v[2];
        g.scan_from = n == 5 ? (uint32_t)v[3] : g.from;
        g.scan_to = n == 5 ? (uint32_t)v[4] : g.to;
        first += g.n_pairs;
        out.push_back(g);
      }
    }
    return out;
  }
  Settings settings() const
  {
    Settings s;
    s.nCU = (int)i("nCU", 256);
    s.hbmBytes = u("hbm", 288000000000ull);
    s.wsLimit = u("wsLimit", 0);
    s.chunkSites = (uint32_t)u("chunkSites", 0);
    s.residentChunks = (int)i("resident", -1);
    s.chunkPool = (int)i("pool", -1);
    s.chunkPoolPhi = (uint32_t)u("phi", 200);
    return s;
  }
  KernelTraits traits() const // (the default: the 69-state member, beta stride 1, built with resident chunks and pool)
  {
    KernelTraits t;
    t.member = (int)i("member", 69);
    t.stride = (int)i("stride", 1);
    t.rowFloat4 = (size_t)u("row4", 18);
    t.sideRows = (size_t)u("side", 4);
    t.chunkFloor = (size_t)u("floor", 512);
    t.resident = i("resBuilt", 1) != 0;
    t.pool = i("poolBuilt", 1) != 0;
    t.perCU = (int)i("perCU", 8);
    return t;
  }
  Diag diag() const
  {
    Diag g;
    g.maxSlots = i("maxSlots", 0);
    g.wavesPerCU = i("wavesPerCU", 0);
    g.sumsSlots = i("sumsSlots", 0);
    g.wsFree = u("wsFree", kFreeWorkspace);
    g.earnScale = d("earnScale", 1.0);
    g.twoWavesNever = i("never", 0) != 0;
    g.w2NW = (int)i("w2nw", 0);
    g.w2KH = (int)i("w2kh", 0);
    return g;
  }
  WsBudget budget() const
  {
    const uint64_t hard = u("hard", 1ull << 30);
    return {hard, u("soft", hard)};
  }
  Credit credit() const
  {
    Credit c;
    c.earned = d("earned", 0);
    c.announced = d("announced", 0);
    c.announcedCredit = d("announcedCredit", 0);
    return c;
  }
  MemInfo mem() const
  {
    MemInfo m;
    m.known = i("memKnown", 1) != 0;
    m.freeBytes = u("memFree", 280000000000ull);
    return m;
  }
};

void printPlan(int rc, const LaunchPlan& p, const std::string& why)
{
  if (rc != FSMC_OK) {
    std::printf("rc=%d why=\"%s\"\n", rc, why.c_str());
    return;
  }
  std::printf("rc=0 chunk=%d chunkRows=%d maxChunks=%d resident=%d wsSlot=%zu slots=%d waves=%d bytes=%zu poolOff=%zu "
              "poolBuffers=%u poolCap=%d\n",
              p.chunk, p.chunkRows, p.maxChunks, p.residentChunks, p.wsSlot, p.slots, p.wavesPerWindow, p.bytes, p.poolOff,
              p.poolBuffers, p.poolCap);
}

void printCredit(const Credit& c)
{
  std::printf("earned=%.17g announced=%.17g announcedCredit=%.17g\n", c.earned, c.announced, c.announcedCredit);
}

void printGroups(const char* name, const std::vector<fsmc_group>& list)
{
  std::printf(" %s=", name);
  for (const fsmc_group& g : list) {
    std::printf("[%u,%u,%u,%u,%u,%u]", g.first_pair, g.n_pairs, g.from, g.to, g.scan_from, g.scan_to);
  }
}

// test_workspace_growth_is_amortised on the CPU: the plan without upgrades gives the base buffer; then `launches`
// launches of one context, each earning a third of that buffer, planned and held the way the library does it (a buffer
// that is too small is replaced by one of the plan's size, and paid for).  Prints the resident chunks of every launch.
void replayGrowth(const Case& c)
{
  const std::vector<fsmc_group> list = c.groups();
  const Settings set = c.settings();
  const KernelTraits k = c.traits();
  const MemInfo mem = c.mem();
  Diag diag = c.diag();
  LaunchPlan plan;
  std::string why;
  Credit credit;
  int rc = planOneWave(set, k, true, list, false, workspaceBudget(set, credit, mem, 0, diag), 1, diag, plan, why);
  const double baseBytes = (double)plan.bytes;
  std::printf("rc=%d baseResident=%d baseBytes=%zu resident=", rc, plan.residentChunks, plan.bytes);
  double pairSites = 0;
  for (const fsmc_group& g : list) {
    pairSites += (double)g.n_pairs * (double)(g.scan_to - g.from);
  }
  diag.earnScale = baseBytes / 3.0 / (kEarnFraction * kernelSeconds(pairSites, (int)c.i("states", 69)) * kAllocBytesPerSecond);
  uint64_t held = 0;
  int allocations = 0;
  for (long l = 0; l < c.i("launches", 24) && rc == FSMC_OK; ++l) {
    earnWorkspace(credit, list, true, (int)c.i("states", 69), diag);
    rc = planOneWave(set, k, true, list, false, workspaceBudget(set, credit, mem, held, diag), 1, diag, plan, why);
    if (rc == FSMC_OK && plan.bytes > held) {
      held = plan.bytes;
      payForWorkspace(set, credit, held, diag);
      ++allocations;
    }
    std::printf("%s%d", l ? "," : "", plan.residentChunks);
  }
  std::printf(" allocations=%d maxChunks=%d\n", allocations, plan.maxChunks);
}

void run(const std::string& fn, const Case& c)
{
  if (fn == "planOneWave") {
    LaunchPlan p;
    std::string why;
    const int rc = planOneWave(c.settings(), c.traits(), c.i("ibd", 1) != 0, c.groups(), c.i("paired", 0) != 0, c.budget(),
                               (unsigned)c.u("share", 1), c.diag(), p, why);
    printPlan(rc, p, why);
  } else if (fn == "planViterbi") {
    LaunchPlan p;
    std::string why;
    const int rc = planViterbi(c.settings(), (int)c.i("S", 640), (int)c.i("member", 69), (int)c.i("perCU", 8),
                               (size_t)c.u("nGroups", 10), c.i("states", 1) != 0, c.budget(), p, why);
    printPlan(rc, p, why);
  } else if (fn == "planSamples") {
    LaunchPlan p;
    std::string why;
    const int rc = planSamples(c.settings(), (int)c.i("S", 640), (int)c.i("member", 69), (int)c.i("perCU", 8),
                               (size_t)c.u("nGroups", 10), c.budget(), p, why);
    printPlan(rc, p, why);
  } else if (fn == "planTwoWaves") {
    LaunchPlan p;
    const size_t nItems = (size_t)c.u("nItems", 10);
    const bool all = allResident(c.settings(), capWorkgroups((int)c.i("counted", 4), 4, 2, c.diag()), nItems);
    const bool fits = planTwoWaves(c.groups(), (int)c.i("member", 69), nItems, c.budget(), p);
    std::printf("allResident=%d fits=%d ", all, fits);
    printPlan(FSMC_OK, p, "");
  } else if (fn == "capWorkgroups") {
    std::printf("perCU=%d\n", capWorkgroups((int)c.i("counted", 8), (int)c.i("most", 8), (int)c.i("divisor", 1), c.diag()));
  } else if (fn == "workspaceBudget") {
    const WsBudget b = workspaceBudget(c.settings(), c.credit(), c.mem(), c.u("cur", 0), c.diag());
    std::printf("hard=%" PRIu64 " soft=%" PRIu64 "\n", b.hard, b.soft);
  } else if (fn == "payForWorkspace") {
    Credit cr = c.credit();
    payForWorkspace(c.settings(), cr, c.u("allocated", 0), c.diag());
    printCredit(cr);
  } else if (fn == "earnWorkspace") {
    Credit cr = c.credit();
    earnWorkspace(cr, c.groups(), c.i("ibd", 1) != 0, (int)c.i("states", 69), c.diag());
    printCredit(cr);
  } else if (fn == "announceLaunchEnd") { // announce a job, launch the list once, then announce 0
    Credit cr = c.credit();
    expectWork(c.settings(), cr, c.d("pairSites", 0), (int)c.i("states", 69), c.diag());
    std::printf("announced: earned=%.17g seconds=%.17g credit=%.17g; ", cr.earned, cr.announced, cr.announcedCredit);
    earnWorkspace(cr, c.groups(), true, (int)c.i("states", 69), c.diag());
    std::printf("launched: earned=%.17g seconds=%.17g credit=%.17g; ended: ", cr.earned, cr.announced, cr.announcedCredit);
    expectWork(c.settings(), cr, 0, (int)c.i("states", 69), c.diag());
    printCredit(cr);
  } else if (fn == "replayGrowth") {
    replayGrowth(c);
  } else if (fn == "staging") {
    const uint64_t limit = stagingLimit(c.settings(), c.mem(), c.u("held", 0), (unsigned)c.u("parts", 1));
    std::printf("limit=%" PRIu64 " stagedItems=%zu keepStrideOne=%d\n", limit,
                stagedItems(limit, (size_t)c.u("perItem", 1), c.diag()),
                sumsKeepStrideOne(c.settings(), (int)c.i("perCU", 8), (size_t)c.u("nBatches", 1)));
  } else if (fn == "planSlices") {
    const std::vector<fsmc_group> list = c.groups();
    Slices s;
    planSlices(list, (size_t)c.u("setting", 0), c.u("stagingBytes", 0), (size_t)c.u("groupBytes", 1),
               c.kv.count("most") ? (size_t)c.u("most", 0) : SIZE_MAX, s);
    const size_t last = s.nSlices - 1;
    std::printf("slice=%zu nSlices=%zu slicePairsMax=%zu last: firstGroup=%zu groups=%zu firstPair=%zu pairs=%zu\n", s.slice,
                s.nSlices, s.slicePairsMax, s.firstGroup(last), s.groups(last), s.firstPair(last), s.pairs(last));
  } else if (fn == "buildDualItems") {
    std::vector<fsmc_group> items, unions, rest;
    const bool dual = buildDualItems(c.groups(), items, unions, rest);
    std::printf("dual=%d", dual);
    if (dual) {
      printGroups("items", items);
      printGroups("unions", unions);
      printGroups("rest", rest);
    }
    std::printf("\n");
  } else if (fn == "longestFirst") {
    std::vector<fsmc_group> list = c.groups();
    const bool moved = longestFirst(list);
    std::printf("reordered=%d", moved);
    printGroups("list", list);
    std::printf("\n");
  } else if (fn == "w2Member") {
    const std::vector<W2Member> built = {{4, 48}, {4, 64}, {4, 80}, {6, 64}, {7, 64}, {8, 64}, {8, 80}, {8, 96}, {8, 128}};
    const W2Member w = w2Member((int)c.i("K", 200), c.diag(), built);
    std::printf("NW=%d KH=%d\n", w.NW, w.KH);
  } else {
    std::printf("unknown function %s\n", fn.c_str());
  }
}
} // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty() || line[0] == '#') {
      continue;
    }
    std::stringstream words(line);
    std::string fn, word;
    words >> fn;
    Case c;
    while (words >> word) {
      const size_t eq = word.find('=');
      if (eq != std::string::npos) {
        c.kv[word.substr(0, eq)] = word.substr(eq + 1);
      }
    }
    run(fn, c);
  }
  return 0;
}
