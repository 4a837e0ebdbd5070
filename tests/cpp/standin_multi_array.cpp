// Checks the stand-in boost::multi_array (oracle/ref_shim/standin/) for the
// properties of Boost.MultiArray the reference DP sources rely on: elements
// value-initialised to zero (also after resize, which keeps the overlap),
// row-major storage, operator[] chains down to an element reference, size()
// on the array and on sub-views is the leading extent, shape() and
// num_elements().  1- to 4-D.  Exits 0 and prints "ok" when all hold.
#include <boost/multi_array.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      ++failures;                                                   \
    }                                                               \
  } while (0)

struct Counted {  // a non-arithmetic element with a value-initialising ctor
  double v;
  Counted() : v(0.0) {}
  Counted(double x) : v(x) {}
};

template <class A>
static bool all_zero(const A& a) {
  for (std::size_t k = 0; k != a.num_elements(); ++k)
    if (a.data()[k] != 0) return false;
  return true;
}

int main() {
  // ---- 1-D
  boost::multi_array<double, 1> a1(boost::extents[7]);
  CHECK(a1.size() == 7 && a1.num_elements() == 7 && a1.shape()[0] == 7 && a1.num_dimensions() == 1);
  CHECK(all_zero(a1));
  a1[3] = 2.5;
  a1[6] += 1.0;
  CHECK(a1.data()[3] == 2.5 && a1.data()[6] == 1.0 && &a1[4] == a1.data() + 4);

  // ---- 2-D, odd extents, a zero extent and a 1 x 1
  boost::multi_array<double, 2> a2(boost::extents[3][5]);
  CHECK(a2.size() == 3 && a2[0].size() == 5 && a2.num_elements() == 15);
  CHECK(a2.shape()[0] == 3 && a2.shape()[1] == 5 && all_zero(a2));
  for (unsigned i = 0; i != 3; ++i)
    for (unsigned j = 0; j != 5; ++j) a2[i][j] = 10.0 * i + j;
  for (unsigned k = 0; k != 15; ++k) CHECK(a2.data()[k] == 10.0 * (k / 5) + k % 5);  // row-major
  CHECK(&a2[2][4] == a2.data() + 14);
  a2[1][2] += a2[0][1] * 2.0;
  CHECK(a2[1][2] == 14.0);
  const boost::multi_array<double, 2>& c2 = a2;
  CHECK(c2[2][3] == 23.0 && c2[1].size() == 5 && c2.size() == 3);
  boost::multi_array<double, 2> copy2(a2);  // deep copy
  copy2[0][0] = -1.0;
  CHECK(a2[0][0] == 0.0 && copy2[2][4] == 24.0 && copy2[0].size() == 5);
  boost::multi_array<double, 2> e2(boost::extents[0][4]);
  CHECK(e2.size() == 0 && e2.num_elements() == 0);
  boost::multi_array<double, 2> one(boost::extents[1][1]);
  CHECK(one.size() == 1 && one[0].size() == 1 && one[0][0] == 0.0);

  // ---- default construction, then resize from empty: all zero
  boost::multi_array<double, 3> a3;
  CHECK(a3.size() == 0 && a3.num_elements() == 0);
  a3.resize(boost::extents[3][4][6]);
  CHECK(a3.size() == 3 && a3[0].size() == 4 && a3[0][0].size() == 6 && a3.num_elements() == 72);
  CHECK(a3.shape()[0] == 3 && a3.shape()[1] == 4 && a3.shape()[2] == 6 && all_zero(a3));
  for (unsigned s = 0; s != 3; ++s)
    for (unsigned i = 0; i != 4; ++i)
      for (unsigned j = 0; j != 6; ++j) a3[s][i][j] = 100.0 * s + 10.0 * i + j;
  CHECK(a3.data()[(2 * 4 + 3) * 6 + 5] == 235.0 && &a3[1][2][3] == a3.data() + (1 * 4 + 2) * 6 + 3);
  const boost::multi_array<double, 3>& c3 = a3;
  CHECK(c3[0].size() == 4 && c3[0][0].size() == 6 && c3[2][1][4] == 214.0);
  // resize keeps the overlap and zero-fills the rest, growing and shrinking
  a3.resize(boost::extents[3][5][4]);
  CHECK(a3.num_elements() == 60 && a3[0].size() == 5 && a3[0][0].size() == 4);
  for (unsigned s = 0; s != 3; ++s)
    for (unsigned i = 0; i != 5; ++i)
      for (unsigned j = 0; j != 4; ++j)
        CHECK(a3[s][i][j] == (i < 4 ? 100.0 * s + 10.0 * i + j : 0.0));
  a3.resize(boost::extents[1][1][1]);
  CHECK(a3.num_elements() == 1 && a3[0][0][0] == 0.0);
  a3.resize(boost::extents[2][2][2]);
  CHECK(all_zero(a3));

  // ---- 3-D of unsigned (the PairHMM's traceback table) and of a class type
  boost::multi_array<unsigned, 3> u3;
  u3.resize(boost::extents[3][2][9]);
  CHECK(all_zero(u3));
  u3[2][1][8] = static_cast<unsigned>(-1);
  CHECK(u3.data()[53] == static_cast<unsigned>(-1));
  boost::multi_array<Counted, 3> k3;
  k3.resize(boost::extents[3][3][2]);
  bool kz = true;
  for (std::size_t k = 0; k != k3.num_elements(); ++k) kz = kz && k3.data()[k].v == 0.0;
  CHECK(kz);
  k3[1][2][1] = static_cast<Counted>(4.0);
  CHECK(k3.data()[(1 * 3 + 2) * 2 + 1].v == 4.0);

  // ---- 4-D (the RIBOSUM pair table)
  boost::multi_array<double, 4> a4(boost::extents[4][3][2][5]);
  CHECK(a4.size() == 4 && a4[0].size() == 3 && a4[0][0].size() == 2 && a4[0][0][0].size() == 5);
  CHECK(a4.num_elements() == 120 && a4.shape()[3] == 5 && all_zero(a4));
  for (unsigned a = 0; a != 4; ++a)
    for (unsigned b = 0; b != 3; ++b)
      for (unsigned c = 0; c != 2; ++c)
        for (unsigned d = 0; d != 5; ++d) a4[a][b][c][d] = ((a * 3 + b) * 2 + c) * 5 + d;
  for (unsigned k = 0; k != 120; ++k) CHECK(a4.data()[k] == k);
  const boost::multi_array<double, 4>& c4 = a4;
  CHECK(c4[3][2][1][4] == 119.0 && c4[1][1].size() == 2);

  // ---- extents built step by step, as `boost::extents[N][n + 1][m + 1]`
  std::vector<int> x(6), y(2);
  boost::multi_array<float, 3> f3(boost::extents[3][x.size() + 1][y.size() + 1]);
  CHECK(f3.size() == 3 && f3[0].size() == 7 && f3[0][0].size() == 3 && all_zero(f3));

  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
