// csrc/bvh4_build.h on the host: build_bvh4's refusal of a BVH deeper than the traversal's stack covers. Prints the number of violations
// (0 = pass). With n_leaf triangles a leaf and the deepest leaf allowed at depth D (root 0) the median split builds n_leaf * 4^D triangles
// and must refuse one more; what it builds must have its deepest leaf at exactly the depth the formula gives, every triangle in exactly
// one leaf, and a refusal must throw before anything else happens to the caller (std::runtime_error naming the limit).
#include <cstdio>
#include <cstring>
#include <functional>
#include "bvh4_build.h"

using namespace ngp;

static std::vector<Triangle> strip(size_t n) { // n small triangles with distinct centroids along a skewed line
	std::vector<Triangle> t(n);
	for (size_t i = 0; i < n; ++i) {
		float x = (float)i * 0.01f, y = (float)((i * 7) % 13) * 0.003f, z = (float)((i * 5) % 11) * 0.002f;
		Triangle tri = {{x, y, z}, {x + 0.004f, y, z}, {x, y + 0.004f, z + 0.001f}};
		t[i] = tri;
	}
	return t;
}

static int depth_and_cover(const std::vector<TriangleBvhNode>& nodes, size_t n_tris, int& bad) {
	std::vector<int> seen(n_tris, 0);
	std::function<int(int, int)> visit = [&](int i, int d) {
		const TriangleBvhNode& nd = nodes[i];
		if (nd.left_idx < 0) {
			for (int k = -nd.left_idx - 1; k < -nd.right_idx - 1; ++k) ++seen[k];
			return d;
		}
		if (nd.right_idx - nd.left_idx != 4) ++bad;
		int deepest = 0;
		for (int c = nd.left_idx; c < nd.left_idx + 4; ++c) deepest = std::max(deepest, visit(c, d + 1));
		return deepest;
	};
	int depth = visit(0, 0);
	for (int s : seen) bad += s != 1;
	return depth;
}

int main() {
	int bad = 0;
	static_assert(3 * BVH4_MAX_DEPTH + 1 <= BVH4_STACK_SIZE, "the deepest BVH the builder lets through fits the traversal's stack");
	static_assert(3 * (BVH4_MAX_DEPTH + 1) + 1 > BVH4_STACK_SIZE, "and one level more would not");
	for (uint32_t leaf : {1u, 3u, 8u}) {
		for (int D = 1; D <= 4; ++D) {
			size_t full = leaf;
			for (int k = 0; k < D; ++k) full *= 4;
			for (size_t n : {full / 4 + 1, full - 1, full}) { // all of these need depth D exactly (full / 4 would still fit depth D - 1)
				std::vector<Triangle> t = strip(n);
				std::vector<TriangleBvhNode> nodes;
				try {
					bvh4::build_bvh4(t, leaf, nodes, D);
					int depth = depth_and_cover(nodes, n, bad);
					if (depth != D) { ++bad; std::printf("leaf %u D %d n %zu: built depth %d\n", leaf, D, n, depth); }
				} catch (const std::exception& e) { ++bad; std::printf("leaf %u D %d n %zu: refused (%s)\n", leaf, D, n, e.what()); }
			}
			std::vector<Triangle> t = strip(full + 1); // one triangle more: some leaf would sit at depth D + 1
			std::vector<TriangleBvhNode> nodes;
			bool threw = false;
			try {
				bvh4::build_bvh4(t, leaf, nodes, D);
			} catch (const std::runtime_error& e) { threw = std::strstr(e.what(), "deeper than") != nullptr; }
			if (!threw) { ++bad; std::printf("leaf %u D %d n %zu: not refused, depth %d\n", leaf, D, full + 1, depth_and_cover(nodes, full + 1, bad)); }
		}
	}
	// the default limit is the stack's: the loader's leaf size with a few levels builds as before
	std::vector<Triangle> t = strip(8 * 64 + 1);
	std::vector<TriangleBvhNode> nodes;
	bvh4::build_bvh4(t, 8, nodes);
	if (depth_and_cover(nodes, t.size(), bad) != 4) ++bad;
	std::printf("%d\n", bad);
	return bad != 0;
}
