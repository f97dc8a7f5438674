// Host replay of the proof walks (khipu_amd/csrc/prove.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_prove_host.py and run as a child process.
//
//   prove_check FILE
// FILE, one record a line:
//   P keyhex valuehex     a put (32-byte keys; "-" = the empty value)
//   Q keyhex              a key to prove and then verify under the trie's root
//   V roothex keyhex n enc_1 .. enc_n [idx]
//                         a proof to verify as given (n node encodings; with idx, one path entry
//                         holding that index instead of the n in order)
// The program builds the canonical records of the trie bottom-up (the builder of
// tests/host_common/replay.h, with export.h's own bodies), then for the Q keys runs the count walk and
// the fill walk of prove.h into arrays of exactly the counted size, encodes every hit through
// export.h's bodies and prints
//   R roothex
//   Q found status valuehex n enc_1 .. enc_n     (status / value: proof_walk over that proof)
// and for every V line
//   V status valuehex
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/prove.h"

// proof_walk over a table built from the encodings (buffers of exactly the needed size; the
// encodings padded to a whole word for the hashing)
static uint8_t verify(const uint8_t* root, const uint8_t* key, const std::vector<Bytes>& nodes,
                      const std::vector<uint32_t>& path, Bytes* value) {
  std::vector<uint64_t> off(nodes.size() + 1, 0), hash(4 * nodes.size() + 1);
  Bytes rlp;
  for (size_t j = 0; j < nodes.size(); ++j) {
    rlp.insert(rlp.end(), nodes[j].begin(), nodes[j].end());
    off[j + 1] = rlp.size();
    kec(nodes[j], &hash[4 * j]);
  }
  if (rlp.empty()) rlp.push_back(0);
  const ProofTable T{rlp.data(), off.data(), hash.data(), nodes.size()};
  const uint8_t* val;
  uint32_t vl;
  const uint8_t st = proof_walk(T, root, key, path.data(), path.size(), &val, &vl);
  value->assign(val, val + vl);
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<Put> in;
  std::vector<Key> queries;
  std::vector<std::string> vlines;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b;
    ss >> tag;
    if (tag == "P" || tag == "Q") {
      ss >> a >> b;
      const Bytes k = unhex(a);
      if (k.size() != 32) return 2;
      Key key;
      memcpy(key.data(), k.data(), 32);
      if (tag == "P")
        in.push_back({key, unhex(b)});
      else
        queries.push_back(key);
    } else if (tag == "V") {
      vlines.push_back(line);
    }
  }
  Builder H(in);
  uint8_t root[32];
  H.root_hash(root);
  printf("R ");
  put_hex(root, 32);
  printf("\n");
  // count walk, scan, fill walk into exactly the counted size
  const size_t nq = queries.size();
  std::vector<uint64_t> pos(nq + 1, 0);
  std::vector<uint8_t> found(nq + 1, 0);
  for (size_t i = 0; i < nq; ++i) {
    uint64_t c = 0;
    found[i] = prove_walk(H.M, H.R, 0, (const uint64_t*)queries[i].data(), [&](uint64_t) { ++c; });
    pos[i + 1] = pos[i] + c;
  }
  uint64_t* hits = new uint64_t[pos[nq]];  // (no slack: a write past the count is ASan's)
  for (size_t i = 0; i < nq; ++i) {
    uint64_t at = pos[i];
    const bool fnd = prove_walk(H.M, H.R, 0, (const uint64_t*)queries[i].data(), [&](uint64_t h) { hits[at++] = h; });
    if (at != pos[i + 1] || fnd != (bool)found[i]) return 6;
  }
  for (size_t i = 0; i < nq; ++i) {
    std::vector<Bytes> nodes;
    std::vector<uint32_t> path;
    for (uint64_t k = pos[i]; k < pos[i + 1]; ++k) {
      path.push_back((uint32_t)nodes.size());
      nodes.push_back(H.encode(hits[k] >> 1, (hits[k] & 1) ? EXP_LOWER : EXP_UPPER));
    }
    Bytes val;
    const uint8_t st = verify(root, queries[i].data(), nodes, path, &val);
    printf("Q %u %u ", (unsigned)found[i], (unsigned)st);
    put_hex(val.data(), val.size());
    printf(" %zu", nodes.size());
    for (const Bytes& e : nodes) {
      printf(" ");
      put_hex(e.data(), e.size());
    }
    printf("\n");
  }
  delete[] hits;
  for (const std::string& vl : vlines) {
    std::istringstream ss(vl);
    std::string tag, rh, kh;
    size_t n;
    ss >> tag >> rh >> kh >> n;
    const Bytes rb = unhex(rh), kb = unhex(kh);
    if (rb.size() != 32 || kb.size() != 32) return 2;
    std::vector<Bytes> nodes;
    std::vector<uint32_t> path;
    for (size_t j = 0; j < n; ++j) {
      std::string e;
      ss >> e;
      nodes.push_back(unhex(e));
      path.push_back((uint32_t)j);
    }
    long idx;
    if (ss >> idx) path.assign(1, (uint32_t)idx);
    Bytes val;
    const uint8_t st = verify(rb.data(), kb.data(), nodes, path, &val);
    printf("V %u ", (unsigned)st);
    put_hex(val.data(), val.size());
    printf("\n");
  }
  return 0;
}
