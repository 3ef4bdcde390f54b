// game::world::WorldBuilder (game/src/world.rs:211-409) as a LevelVisitor.  See game_world.hpp.
#include "game_world.hpp"

#include <algorithm>
#include <cmath>
#include <map>

namespace rdoom::game {
using namespace rdoom::wad;

namespace {
class WorldBuilder : public LevelVisitor {
 public:
  void visit_bsp_root(const Line2f &line) override {  // world.rs:312-316
    if (!nodes_.empty()) throw WadError(RDOOM_BAD_LEVEL, "world: a second BSP root");
    nodes_.push_back(node(line));
    stack_.push_back(0);
    depth_ = std::max<uint32_t>(depth_, 1);
  }
  void visit_bsp_node(const Line2f &line, Branch branch) override {  // world.rs:318-323
    const int32_t index = (int32_t)nodes_.size();
    nodes_.push_back(node(line));
    link_child(index, branch);
    stack_.push_back((uint32_t)index);
    depth_ = std::max<uint32_t>(depth_, (uint32_t)stack_.size());
  }
  void visit_bsp_leaf(Branch branch) override {  // world.rs:325-332
    const uint32_t index = (uint32_t)chunks_.size();
    const uint32_t n = (uint32_t)triangles_[0].size();
    chunks_.push_back({n, n});
    link_child(-(int32_t)index, branch);  // Child::Leaf(index).pack()
  }
  void visit_bsp_leaf_end() override {  // world.rs:334-337
    if (chunks_.empty()) throw WadError(RDOOM_BAD_LEVEL, "world: leaf end without a leaf");
    chunks_.back().tri_end = (uint32_t)triangles_[0].size();
  }
  void visit_bsp_node_end() override {  // world.rs:339-344
    if (stack_.empty()) throw WadError(RDOOM_BAD_LEVEL, "world: too many BSP node ends");
    stack_.pop_back();
  }
  void visit_floor_sky_poly(const SkyPoly &p) override { floor(p.object_id, p.vertices, p.n_vertices, p.height); }
  void visit_ceil_sky_poly(const SkyPoly &p) override { ceil(p.object_id, p.vertices, p.n_vertices, p.height); }
  void visit_floor_poly(const StaticPoly &p) override { floor(p.object_id, p.vertices, p.n_vertices, p.height); }
  void visit_ceil_poly(const StaticPoly &p) override { ceil(p.object_id, p.vertices, p.n_vertices, p.height); }
  void visit_wall_quad(const StaticQuad &q) override {  // world.rs:380-388: only blockers collide
    if (q.blocker) quad(q.object_id, q.v1, q.v2, q.height_range);
  }
  void visit_sky_quad(const SkyQuad &q) override { quad(q.object_id, q.v1, q.v2, q.height_range); }
  void visit_marker(const float pos[3], float yaw, Marker marker) override { start_from_marker(pos, yaw, marker, start_pos_, start_yaw_); }

  World build() {  // world.rs:230-258: object 0's triangles, then one dynamic chunk per other object, by ascending id
    World w;
    if (nodes_.empty()) throw WadError(RDOOM_BAD_LEVEL, "world: the level has no BSP nodes");
    w.nodes = std::move(nodes_);
    w.chunks = std::move(chunks_);
    w.verts = std::move(verts_);
    for (auto &kv : triangles_) {
      const uint32_t start = (uint32_t)w.triangles.size();
      w.triangles.insert(w.triangles.end(), kv.second.begin(), kv.second.end());
      if (kv.first > 0) {
        w.dynamics.push_back({kv.first, start, (uint32_t)w.triangles.size()});
        w.n_objects = std::max(w.n_objects, kv.first + 1);
      } else {
        w.n_static_triangles = (uint32_t)w.triangles.size();
      }
    }
    w.node_depth = depth_;
    std::copy(start_pos_, start_pos_ + 3, w.start_pos);
    w.start_yaw = start_yaw_;
    return w;
  }

 private:
  static WorldNode node(const Line2f &l) {  // Node::new (world.rs:166-172)
    return WorldNode{{l.origin.x, l.origin.y}, {l.displace.x, l.displace.y}, l.length, 0, 0};
  }
  void link_child(int32_t packed, Branch branch) {  // world.rs:261-279 (the reference asserts the slot is still 0)
    if (stack_.empty()) throw WadError(RDOOM_BAD_LEVEL, "world: link_child on the root");
    WorldNode &parent = nodes_[stack_.back()];
    int32_t &slot = branch == Branch::Positive ? parent.positive : parent.negative;
    if (slot != 0) throw WadError(RDOOM_BAD_LEVEL, "world: a BSP child linked twice");
    slot = packed;
  }
  // add_polygon (world.rs:281-305): the vertices, then the normal as one more vertex, and a fan over them
  void add_polygon(ObjectId object, const float *xyz, size_t n, const float normal[3]) {
    std::vector<WorldTriangle> &tris = triangles_[object.v];
    const uint32_t start = (uint32_t)(verts_.size() / 3);
    verts_.insert(verts_.end(), xyz, xyz + 3 * n);
    const uint32_t end = (uint32_t)(verts_.size() / 3);
    verts_.insert(verts_.end(), normal, normal + 3);
    for (uint32_t i = start + 2; i < end; i++) tris.push_back({start, i - 1, i, end});
  }
  void floor(ObjectId object, const Pnt2f *v, size_t n, float height) {  // world.rs:346-355
    scratch_.clear();
    for (size_t i = 0; i < n; i++) scratch_.insert(scratch_.end(), {v[i].x, height, v[i].y});
    const float up[3] = {0.0f, 1.0f, 0.0f};
    add_polygon(object, scratch_.data(), n, up);
  }
  void ceil(ObjectId object, const Pnt2f *v, size_t n, float height) {  // world.rs:357-367: reversed
    scratch_.clear();
    for (size_t i = n; i-- > 0;) scratch_.insert(scratch_.end(), {v[i].x, height, v[i].y});
    const float down[3] = {0.0f, -1.0f, 0.0f};
    add_polygon(object, scratch_.data(), n, down);
  }
  void quad(ObjectId object, Pnt2f v1, Pnt2f v2, const float range[2]) {  // world.rs:390-408
    // (v2 - v1).normalize_or_zero(): v / max(|v|, f32::EPSILON) (math/src/lib.rs:40-42)
    const float ex = v2.x - v1.x, ey = v2.y - v1.y;
    const float m = std::sqrt(ex * ex + ey * ey);
    const float d = m > 1.1920929e-7f ? m : 1.1920929e-7f;
    const float nx = ex / d, ny = ey / d;
    const float normal[3] = {-ny, 0.0f, nx};
    const float low = range[0], high = range[1];
    const float xyz[12] = {v1.x, low, v1.y, v2.x, low, v2.y, v2.x, high, v2.y, v1.x, high, v1.y};
    add_polygon(object, xyz, 4, normal);
  }

  std::vector<WorldNode> nodes_;
  std::vector<WorldChunk> chunks_;
  std::vector<float> verts_, scratch_;
  std::vector<uint32_t> stack_;
  std::map<uint32_t, std::vector<WorldTriangle>> triangles_{{0u, {}}};  // VecMap<Vec<Triangle>>: iterated by ascending key
  uint32_t depth_ = 0;
  float start_pos_[3] = {0, 0, 0}, start_yaw_ = 0.0f;
};
}  // namespace

World build_world(const LoadedWad &w, size_t level_index) {
  const Archive &archive = *w.archive;  // walk_level, keeping the analysis for the triggers
  const Level level = Level::from_archive(archive, level_index);
  const LevelAnalysis analysis(level, archive.metadata());
  WorldBuilder b;
  std::vector<uint32_t> leaf_subsectors;  // per chunk, in walk order
  std::vector<rdoom_thing> things;        // the thing table, in lump order
  {
    LevelWalker walker(level, analysis, w.textures, archive.metadata(), b);
    walker.record_leaf_subsectors = &leaf_subsectors;
    walker.record_things = &things;
    walker.walk();
  }
  World out = b.build();
  out.things = std::move(things);
  out.thing_obstacles.assign(std::max<size_t>(1, (out.things.size() + 31) / 32), 0u);
  for (size_t i = 0; i < out.things.size(); i++) {  // the entry that gave the record its category: the first match
    const ThingMetadata *m = archive.metadata().find_thing(out.things[i].thing_type);
    if (m && m->obstacle) out.thing_obstacles[i / 32] |= 1u << (i % 32);
  }
  out.game_objects = (uint32_t)std::max<size_t>(1, analysis.num_objects());
  for (const Trigger &t : analysis.triggers()) {
    rdoom_trigger r{};
    r.origin[0] = t.line.origin.x, r.origin[1] = t.line.origin.y;
    r.displace[0] = t.line.displace.x, r.displace[1] = t.line.displace.y;
    r.length = t.line.length;
    r.trigger_type = (uint32_t)t.type;
    r.flags = (t.only_once ? RDOOM_TRIGGER_ONLY_ONCE : 0u) | (t.exit ? RDOOM_TRIGGER_EXIT : 0u) |
              (t.unimplemented ? RDOOM_TRIGGER_UNIMPLEMENTED : 0u);
    r.special_type = t.special_type;
    r.effect_start = (uint32_t)out.effects.size();
    for (const MoveEffect &e : t.effects)
      out.effects.push_back(rdoom_move_effect{e.object_id.v, e.first_height_offset, e.second_height_offset.value_or(0.0f), e.speed, e.wait,
                                              e.second_height_offset.has_value(), e.repeat});
    r.effect_end = (uint32_t)out.effects.size();
    out.triggers.push_back(r);
  }
  // the map's line table: every linedef whose two vertices exist, in linedef order (wad/src/types.rs:49-57 WadLinedef;
  // wad/src/level.rs:83-87, 131-151 vertex / left_sidedef / right_sidedef / sidedef_sector), each side with its sector's heights and the
  // floor and ceiling objects SectorInfo gives it (wad/src/visitor.rs:145-156, 569-588: 0 unless a DynamicSectorInfo moves it)
  for (size_t i = 0; i < level.linedefs.size(); i++) {
    const WadLinedef &l = level.linedefs[i];
    const auto a = level.vertex(l.start_vertex), b = level.vertex(l.end_vertex);
    if (!a || !b) continue;
    rdoom_map_line m{};
    m.linedef = (uint32_t)i;
    m.a[0] = a->x, m.a[1] = a->y, m.b[0] = b->x, m.b[1] = b->y;
    m.flags = l.flags, m.special_type = l.special_type;
    const auto side = [&](int16_t index) {
      rdoom_map_side s{};
      const WadSector *sector = level.sidedef_sector(level.side(index));
      if (!sector) return s;
      s.present = 1;
      s.floor = from_wad_height(sector->floor_height), s.ceiling = from_wad_height(sector->ceiling_height);
      if (const DynamicSectorInfo *d = analysis.dynamic(level.sector_id(sector))) s.floor_id = d->floor_id.v, s.ceiling_id = d->ceiling_id.v;
      return s;
    };
    m.front = side(l.right_side), m.back = side(l.left_side);
    out.map_lines.push_back(m);
  }
  // the sector table: every sector in lump order, with the heights and objects the line table gives its sides
  for (const WadSector &sc : level.sectors) {
    rdoom_map_sector r{};
    r.floor = from_wad_height(sc.floor_height), r.ceiling = from_wad_height(sc.ceiling_height);
    if (const DynamicSectorInfo *d = analysis.dynamic(level.sector_id(&sc))) r.floor_id = d->floor_id.v, r.ceiling_id = d->ceiling_id.v;
    r.light_level = (uint16_t)sc.light, r.sector_type = sc.sector_type, r.tag = sc.tag;
    out.map_sectors.push_back(r);
  }
  // per chunk the sector of its sub-sector -- of its first seg, as LevelWalker::subsector picks it -- and the solid edges: the segs
  // with nothing behind them, start vertex and end - start.  Chunk 0 exists for the descent even when the walk met no leaf.
  const size_t n_leaves = std::max<size_t>(1, out.chunks.size());
  out.leaf_sector.assign(n_leaves, RDOOM_SECTOR_NONE);
  out.leaf_edges.assign(n_leaves, rdoom_map_leaf_edges{0, 0});
  for (size_t k = 0; k < leaf_subsectors.size() && k < n_leaves; k++) {
    out.leaf_edges[k].first = (uint32_t)out.map_edges.size();
    if (leaf_subsectors[k] == LevelWalker::NO_SUBSECTOR) continue;
    const WadSubsector ss = level.subsectors[leaf_subsectors[k]];
    const WadSeg *segs = &level.segs[ss.first_seg];
    out.leaf_sector[k] = level.sector_id(level.seg_sector(segs[0]));
    for (size_t i = 0; i < ss.num_segs; i++) {
      if (!level.seg_linedef(segs[i]) || level.seg_back_sidedef(segs[i])) continue;
      const Pnt2f a = *level.vertex(segs[i].start_vertex), e = *level.vertex(segs[i].end_vertex);
      out.map_edges.push_back(rdoom_map_edge{{a.x, a.y}, {e.x - a.x, e.y - a.y}});
    }
    out.leaf_edges[k].count = (uint32_t)out.map_edges.size() - out.leaf_edges[k].first;
  }
  out.spawn = build_spawn_table(out);
  return out;
}

std::vector<rdoom_spawn_entry> build_spawn_table(const World &w) {
  std::vector<rdoom_spawn_entry> out;
  double sum = 0.0;
  for (const WorldTriangle &t : w.triangles) {
    if (!(w.verts[(size_t)t.normal * 3 + 1] > 0.0f)) continue;  // floors only: walls have y == 0, ceilings y < 0
    const float *a = &w.verts[(size_t)t.v1 * 3], *b = &w.verts[(size_t)t.v2 * 3], *c = &w.verts[(size_t)t.v3 * 3];
    const double ux = (double)b[0] - (double)a[0], uz = (double)b[2] - (double)a[2];
    const double vx = (double)c[0] - (double)a[0], vz = (double)c[2] - (double)a[2];
    const double area = 0.5 * std::fabs(ux * vz - uz * vx);
    if (!(area > 0.0)) continue;
    sum += area;
    out.push_back(rdoom_spawn_entry{{a[0], a[1], a[2]}, {b[0], b[1], b[2]}, {c[0], c[1], c[2]}, (float)sum});
  }
  return out;
}

WorldSet build_world_set(const LoadedWad &w, const uint32_t *level_indices, size_t n) {
  if (!n || !level_indices) throw WadError(RDOOM_BAD_ARG, "world set: no levels");
  const size_t n_archive = w.archive->num_levels();
  std::map<uint32_t, uint32_t> slot_of;
  for (size_t s = 0; s < n; s++) {
    if (level_indices[s] >= n_archive) throw WadError(RDOOM_BAD_ARG, "world set: level index out of range");
    if (!slot_of.emplace(level_indices[s], (uint32_t)s).second) throw WadError(RDOOM_BAD_ARG, "world set: a level index twice");
  }
  WorldSet set;
  World &all = set.all;
  all.n_objects = 0;
  for (size_t s = 0; s < n; s++) {
    set.levels.push_back(build_world(w, level_indices[s]));
    const World &l = set.levels.back();
    WorldSetLevel t{};
    t.archive_index = level_indices[s];
    const auto next = slot_of.find(level_indices[s] + 1);
    t.destination = next == slot_of.end() ? NO_DESTINATION : next->second;
    t.node_base = (uint32_t)all.nodes.size(), t.chunk_base = (uint32_t)all.chunks.size();
    t.triangle_base = (uint32_t)all.triangles.size(), t.vert_base = (uint32_t)(all.verts.size() / 3);
    t.dynamic_base = (uint32_t)all.dynamics.size(), t.trigger_base = (uint32_t)all.triggers.size();
    t.effect_base = (uint32_t)all.effects.size(), t.map_base = (uint32_t)all.map_lines.size();
    for (WorldNode nd : l.nodes) {
      for (int32_t *c : {&nd.positive, &nd.negative}) *c = *c > 0 ? *c + (int32_t)t.node_base : *c - (int32_t)t.chunk_base;
      all.nodes.push_back(nd);
    }
    for (const WorldChunk &c : l.chunks) all.chunks.push_back({c.tri_start + t.triangle_base, c.tri_end + t.triangle_base});
    for (const WorldTriangle &tr : l.triangles)
      all.triangles.push_back({tr.v1 + t.vert_base, tr.v2 + t.vert_base, tr.v3 + t.vert_base, tr.normal + t.vert_base});
    all.verts.insert(all.verts.end(), l.verts.begin(), l.verts.end());
    for (const WorldDynamic &d : l.dynamics) all.dynamics.push_back({d.object_id, d.tri_start + t.triangle_base, d.tri_end + t.triangle_base});
    for (rdoom_trigger tr : l.triggers) {
      tr.effect_start += t.effect_base, tr.effect_end += t.effect_base;
      all.triggers.push_back(tr);
    }
    all.effects.insert(all.effects.end(), l.effects.begin(), l.effects.end());
    all.map_lines.insert(all.map_lines.end(), l.map_lines.begin(), l.map_lines.end());
    all.n_objects = std::max(all.n_objects, l.n_objects);
    set.game_objects = std::max(set.game_objects, l.game_objects);
    set.node_depth = std::max(set.node_depth, l.node_depth);
    set.table.push_back(t);
  }
  all.game_objects = set.game_objects, all.node_depth = set.node_depth;
  return set;
}

}  // namespace rdoom::game
