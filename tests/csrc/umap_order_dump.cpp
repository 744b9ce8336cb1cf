// Prints the iteration order of a real std::unordered_map<int, int>.  Stand-alone: nothing of the project's is included.
// stdin, one experiment per line:   k1 k2 ... kn [; e1 e2 ... em]
// stdout per experiment: a line "=" followed by the keys in iteration order after the n insertions (operator[], in the order given),
// one more such line after each erase(e), then a line ".".
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>

static void dump(const std::unordered_map<int, int>& m) {
  std::cout << "=";
  for (auto it = m.begin(); it != m.end(); ++it) std::cout << " " << it->first;
  std::cout << "\n";
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::unordered_map<int, int> m;
    const size_t semi = line.find(';');
    std::istringstream ins(line.substr(0, semi)), del(semi == std::string::npos ? std::string() : line.substr(semi + 1));
    int k;
    while (ins >> k) m[k] = 1;
    dump(m);
    while (del >> k) {
      m.erase(k);
      dump(m);
    }
    std::cout << ".\n";
  }
  return 0;
}
