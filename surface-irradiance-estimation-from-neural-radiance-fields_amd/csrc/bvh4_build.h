// The BVH4 of a triangle mesh: its node and triangle layout, the traversal's stack bound and the host-side builder. Plain C++ without a
// HIP header, so that tests/aux/bvh4_depth_check.cpp can build it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <limits>
#include <stack>
#include <stdexcept>
#include <string>
#include <vector>

namespace ngp {

struct Triangle { // triangle.cuh:163 -- 36 B
	float a[3], b[3], c[3];
};
struct TriangleBvhNode { // triangle_bvh.cuh:28-32 -- 32 B
	float bmin[3], bmax[3];
	int left_idx; // negative: leaf, triangles [-left_idx-1, -right_idx-1)
	int right_idx;
};
// The traversal keeps the nodes it still has to visit on a fixed stack. Popping a node pushes at most its four children, so with the
// deepest leaf at depth D (root 0) the stack never holds more than 3 D + 1 entries. build_bvh4 refuses a mesh deeper than BVH4_MAX_DEPTH;
// its median split puts at most 8 * 4^D triangles at depth D, so that takes more than 8 * 4^10 (8.4 million) triangles.
constexpr int BVH4_STACK_SIZE = 32;
constexpr int BVH4_MAX_DEPTH = (BVH4_STACK_SIZE - 1) / 3;

namespace bvh4 {

struct V3 {
	float x, y, z;
};
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator*(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
inline V3 operator/(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
inline V3 vmin(V3 a, V3 b) { return {std::min(a.x, b.x), std::min(a.y, b.y), std::min(a.z, b.z)}; }
inline V3 vmax(V3 a, V3 b) { return {std::max(a.x, b.x), std::max(a.y, b.y), std::max(a.z, b.z)}; }
inline V3 ld(const float* p) { return {p[0], p[1], p[2]}; }
inline void st(float* p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

inline V3 centroid(const Triangle& t) { return (ld(t.a) + ld(t.b) + ld(t.c)) / 3.0f; }           // triangle.cuh:149-151
inline float centroid(const Triangle& t, int axis) { return (t.a[axis] + t.b[axis] + t.c[axis]) / 3; } // triangle.cuh:153-155

inline void bounds(const Triangle* begin, const Triangle* end, float* bmin, float* bmax) { // BoundingBox(Triangle*, Triangle*)
	V3 lo = ld(begin->a), hi = lo;
	for (const Triangle* it = begin; it != end; ++it) {
		lo = vmin(lo, vmin(ld(it->a), vmin(ld(it->b), ld(it->c))));
		hi = vmax(hi, vmax(ld(it->a), vmax(ld(it->b), ld(it->c))));
	}
	st(bmin, lo);
	st(bmax, hi);
}

// TriangleBvhWithBranchingFactor<4>::build (src/triangle_bvh.cu:425-508)
// max_depth: the deepest leaf allowed (root 0); a mesh that needs a deeper one is refused, nothing is dropped or truncated
inline void build_bvh4(std::vector<Triangle>& triangles, uint32_t n_primitives_per_leaf, std::vector<TriangleBvhNode>& nodes, int max_depth = BVH4_MAX_DEPTH) {
	constexpr int BF = 4;
	nodes.clear();
	nodes.emplace_back();
	bounds(triangles.data(), triangles.data() + triangles.size(), nodes.front().bmin, nodes.front().bmax);
	nodes.front().left_idx = nodes.front().right_idx = 0;
	struct BuildNode {
		int node_idx;
		int depth;
		std::vector<Triangle>::iterator begin, end;
	};
	std::stack<BuildNode> build_stack;
	build_stack.push({0, 0, triangles.begin(), triangles.end()});
	while (!build_stack.empty()) {
		BuildNode curr = build_stack.top();
		build_stack.pop();
		std::array<BuildNode, BF> children;
		children[0].begin = curr.begin;
		children[0].end = curr.end;
		int n_children = 1;
		while (n_children < BF) {
			for (int i = n_children - 1; i >= 0; --i) {
				BuildNode child = children[i];
				const float count = (float)std::distance(child.begin, child.end);
				V3 mean{0.f, 0.f, 0.f};
				for (auto it = child.begin; it != child.end; ++it) mean = mean + centroid(*it);
				mean = mean / count;
				V3 var{0.f, 0.f, 0.f};
				for (auto it = child.begin; it != child.end; ++it) {
					V3 diff = centroid(*it) - mean;
					var = var + diff * diff;
				}
				var = var / count;
				float max_val = std::max(std::max(var.x, var.y), var.z);
				int axis = var.x == max_val ? 0 : (var.y == max_val ? 1 : 2);
				auto m = child.begin + std::distance(child.begin, child.end) / 2;
				std::nth_element(child.begin, m, child.end, [&](const Triangle& t1, const Triangle& t2) { return centroid(t1, axis) < centroid(t2, axis); });
				children[i * 2].begin = child.begin;
				children[i * 2 + 1].end = child.end;
				children[i * 2].end = children[i * 2 + 1].begin = m;
			}
			n_children *= 2;
		}
		nodes[curr.node_idx].left_idx = (int)nodes.size();
		for (int i = 0; i < BF; ++i) {
			BuildNode& child = children[i];
			child.node_idx = (int)nodes.size();
			nodes.emplace_back();
			TriangleBvhNode& nd = nodes.back();
			if (child.begin != child.end) {
				bounds(&*child.begin, &*child.begin + std::distance(child.begin, child.end), nd.bmin, nd.bmax);
			} else { // the reference asserts this away; an empty child is an empty leaf
				for (int k = 0; k < 3; ++k) { nd.bmin[k] = std::numeric_limits<float>::infinity(); nd.bmax[k] = -std::numeric_limits<float>::infinity(); }
			}
			if (std::distance(child.begin, child.end) <= (std::ptrdiff_t)n_primitives_per_leaf) {
				nd.left_idx = -(int)std::distance(triangles.begin(), child.begin) - 1;
				nd.right_idx = -(int)std::distance(triangles.begin(), child.end) - 1;
			} else {
				nd.left_idx = nd.right_idx = 0;
				child.depth = curr.depth + 1;
				// the children of this node would sit below what the traversal's stack covers (it would drop nodes without a word)
				if (child.depth + 1 > max_depth)
					throw std::runtime_error("mesh too large: its BVH would be deeper than " + std::to_string(max_depth) + " levels (the traversal stack of " + std::to_string(BVH4_STACK_SIZE) +
					                         " entries covers " + std::to_string(BVH4_MAX_DEPTH) + "); a mesh may hold at most " + std::to_string(n_primitives_per_leaf) + " * 4^" + std::to_string(max_depth) + " triangles");
				build_stack.push(child);
			}
		}
		nodes[curr.node_idx].right_idx = (int)nodes.size();
	}
}

} // namespace bvh4
} // namespace ngp
