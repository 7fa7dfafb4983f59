// CPU slice of the WRMF confidence weights for tests/test_als_weighted_reference.py: the SAME header cdae_hip.hip compiles
// (cdae_amd/csrc/cdae_dataset_plan.h) behind a C ABI for ctypes.  Test infrastructure.
#include <cstring>

#include "../../cdae_amd/csrc/cdae_dataset_plan.h"

using namespace cdae;

extern "C" {

// the item-major CSR of item_major_csr (ptr [I + 1], col [nnz]) and the weights carried through the same counting sort (tw [nnz])
void aw_item_major(uint64_t U, uint64_t I, const int64_t* row_ptr, const uint32_t* col, const float* w, int64_t* ptr, uint32_t* tcol, float* tw) {
  std::vector<uint64_t> pop;
  (void)plan::check_rows(U, I, row_ptr, col, false, false, pop);
  const plan::ItemMajor t = plan::item_major_csr(U, I, row_ptr, col, pop);
  const std::vector<float> v = plan::item_major_weights(U, I, row_ptr, col, w);
  const size_t nnz = (size_t)row_ptr[U];
  std::memcpy(ptr, t.ptr.data(), (I + 1) * sizeof(int64_t));
  if (nnz) { std::memcpy(tcol, t.col.data(), nnz * sizeof(uint32_t)); std::memcpy(tw, v.data(), nnz * sizeof(float)); }
}

// check_weights: the length of the refusal's text (0: accepted), the text itself in err
size_t aw_check_weights(const float* w, size_t count, char* err, size_t err_cap) {
  const std::string e = plan::check_weights(w, count);
  std::snprintf(err, err_cap, "%s", e.c_str());
  return e.size();
}

}
