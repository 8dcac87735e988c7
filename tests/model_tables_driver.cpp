// model_tables_driver.cpp -- fsmc_model_tables.h on a CPU: reads cases from stdin, one a line, and prints each result on
// one line (tests/test_model_tables.py holds the cases and what they must give).
//
// A case is a function's name and key=value inputs.  Float arrays go in and come out as the 32-bit patterns of their
// elements, hexadecimal, comma separated: nothing is rounded on the way, and -0.0 is not +0.0.
//
// checkDesc starts from a description that passes (K = 3, S = 4, two table rows; sequence=1: with the sequence-mode
// arrays) and applies the case's changes: K=, S=, n_rows=, state_threshold=, age_threshold=, null=<field>,
// <row array>=<site>:<value>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "fsmc_model_tables.h"

using namespace fsmc;

namespace
{
struct Case {
  std::map<std::string, std::string> kv;
  bool has(const char* key) const { return kv.count(key) != 0; }
  long i(const char* key, long dflt) const
  {
    const auto it = kv.find(key);
    return it == kv.end() ? dflt : std::atol(it->second.c_str());
  }
  std::vector<std::string> items(const char* key, char sep = ',') const
  {
    std::vector<std::string> out;
    const auto it = kv.find(key);
    if (it != kv.end()) {
      std::stringstream all(it->second);
      std::string one;
      while (std::getline(all, one, sep)) {
        out.push_back(one);
      }
    }
    return out;
  }
  std::vector<float> floats(const char* key) const
  {
    std::vector<float> out;
    for (const std::string& w : items(key)) {
      const uint32_t bits = (uint32_t)std::strtoul(w.c_str(), nullptr, 16);
      float f;
      std::memcpy(&f, &bits, sizeof(f));
      out.push_back(f);
    }
    return out;
  }
  std::vector<int32_t> ints(const char* key) const
  {
    std::vector<int32_t> out;
    for (const std::string& w : items(key)) {
      out.push_back((int32_t)std::atol(w.c_str()));
    }
    return out;
  }
};

void printFloats(const std::vector<float>& v)
{
  std::printf("n=%zu bits=", v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    uint32_t bits;
    std::memcpy(&bits, &v[i], sizeof(bits));
    std::printf("%s%08x", i ? "," : "", bits);
  }
  std::printf("\n");
}

void printStatus(int rc, const std::string& why)
{
  if (rc == FSMC_OK) {
    std::printf("rc=0\n");
  } else {
    std::printf("rc=%d why=\"%s\"\n", rc, why.c_str());
  }
}

void checkDesc(const Case& c)
{
  fsmc_model_desc d;
  std::memset(&d, 0, sizeof(d));
  d.K = (int32_t)c.i("K", 3);
  d.S = (int32_t)c.i("S", 4);
  d.n_rows = (int32_t)c.i("n_rows", 2);
  d.state_threshold = (uint32_t)c.i("state_threshold", 1);
  d.age_threshold = (uint32_t)c.i("age_threshold", 1);
  d.sequence = (int32_t)c.i("sequence", 0);
  const std::vector<float> table(64, 0.5f);
  // (entry 0 of a row array is never read: out of range here, and the description still passes)
  std::map<std::string, std::vector<int32_t>> rowArrays;
  for (const char* name : {"step_row", "gap_row_f", "site_row_f", "gap_row_b", "site_row_b"}) {
    rowArrays[name] = {-7, 0, 1, 1, 0, 1, 0, 1};
    for (const std::string& change : c.items(name)) {
      const size_t colon = change.find(':');
      rowArrays[name][(size_t)std::atol(change.c_str())] = (int32_t)std::atol(change.c_str() + colon + 1);
    }
  }
  std::map<std::string, const float**> floatFields = {
      {"pi", &d.pi}, {"col_ratios", &d.col_ratios}, {"exp_times", &d.exp_times}, {"D", &d.D}, {"B", &d.B}, {"U", &d.U},
      {"RR", &d.RR}, {"e1", &d.e1}, {"e0m1", &d.e0m1}, {"e2m0", &d.e2m0}, {"hom", &d.hom}};
  std::map<std::string, const int32_t**> rowFields = {{"step_row", &d.step_row},
                                                      {"gap_row_f", &d.gap_row_f},
                                                      {"site_row_f", &d.site_row_f},
                                                      {"gap_row_b", &d.gap_row_b},
                                                      {"site_row_b", &d.site_row_b}};
  const bool seq = d.sequence != 0;
  for (auto& f : floatFields) {
    *f.second = (f.first != "hom" || seq) ? table.data() : nullptr;
  }
  for (auto& f : rowFields) {
    *f.second = (f.first == "step_row" || seq) ? rowArrays[f.first].data() : nullptr;
  }
  for (const std::string& name : c.items("null")) {
    if (floatFields.count(name)) {
      *floatFields[name] = nullptr;
    } else if (rowFields.count(name)) {
      *rowFields[name] = nullptr;
    } else {
      std::printf("unknown field %s\n", name.c_str());
      return;
    }
  }
  std::string why;
  const int rc = model::checkDesc(d, why);
  printStatus(rc, why);
}

// groups=<n_pairs>:<first_pair>:<from>:<to>:<scan_from>:<scan_to>,...
void checkWorklist(const Case& c)
{
  std::vector<fsmc_group> groups;
  for (const std::string& one : c.items("groups")) {
    unsigned long v[6] = {0, 0, 0, 0, 0, 0};
    std::sscanf(one.c_str(), "%lu:%lu:%lu:%lu:%lu:%lu", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]);
    fsmc_group g;
    g.n_pairs = (uint32_t)v[0];
    g.first_pair = (uint32_t)v[1];
    g.from = (uint32_t)v[2];
    g.to = (uint32_t)v[3];
    g.scan_from = (uint32_t)v[4];
    g.scan_to = (uint32_t)v[5];
    groups.push_back(g);
  }
  std::string why;
  const int rc = model::checkWorklist((size_t)std::strtoull(c.kv.at("n_pairs").c_str(), nullptr, 10), groups.data(),
                                      groups.size(), why);
  printStatus(rc, why);
}

void run(const std::string& fn, const Case& c)
{
  const int K = (int)c.i("K", 0), KP = (int)c.i("KP", 0);
  if (fn == "shapeOf") {
    plan::Diag diag;
    diag.w2NW = (int)c.i("w2nw", 0);
    diag.w2KH = (int)c.i("w2kh", 0);
    const std::vector<plan::W2Member> built = {{4, 48}, {4, 64}, {4, 80}, {6, 64}, {7, 64}, {8, 64}, {8, 80}, {8, 96}, {8, 128}};
    const model::Shape s = model::shapeOf(K, diag, built);
    std::printf("KP=%d w2NW=%d\n", s.KP, s.w2NW);
  } else if (fn == "checkDesc") {
    checkDesc(c);
  } else if (fn == "checkWorklist") {
    checkWorklist(c);
  } else if (fn == "padRows") {
    printFloats(model::padRows(c.floats("src").data(), (size_t)c.i("rows", 1), K, KP));
  } else if (fn == "rowSets") {
    printFloats(model::rowSets(c.floats("D").data(), c.floats("B").data(), c.floats("U").data(), c.floats("RR").data(),
                               (size_t)c.i("rows", 1), K, KP));
  } else if (fn == "ghostMask") {
    printFloats(model::ghostMask(K, KP));
  } else if (fn == "stepRows") {
    const std::vector<int32_t> src = c.ints("src");
    const std::vector<int> rows = model::stepRows(src.data(), (int32_t)src.size());
    std::printf("n=%zu rows=", rows.size());
    for (size_t i = 0; i < rows.size(); ++i) {
      std::printf("%s%d", i ? "," : "", rows[i]);
    }
    std::printf("\n");
  } else if (fn == "emissions") {
    const std::vector<float> e1 = c.floats("e1"), e0m1 = c.floats("e0m1"), e2m0 = c.floats("e2m0"), hom = c.floats("hom");
    fsmc_model_desc d;
    std::memset(&d, 0, sizeof(d));
    d.K = K;
    d.S = (int32_t)c.i("S", 1);
    d.e1 = e1.data();
    d.e0m1 = e0m1.data();
    d.e2m0 = e2m0.data();
    d.sequence = (int32_t)c.i("sequence", 0);
    d.hom = d.sequence ? hom.data() : nullptr;
    printFloats(model::emissions(d, KP));
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
