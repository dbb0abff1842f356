"""The packet-culling certificates applied to NODES of 4, 16 or 64 consecutive tiles (rt_mfma.hpp `prepare_cull_kernel`
with `rec_tris` = 10 x node size, rt_scan.hpp `packet_cull_kernel` pass 1), on the CPU.

A node record is the tile record of the union of its triangles: every bound is a min or a max over the set, so a certificate that
fires for the node is a certificate for every triangle of it.  This file restates that record in fp32 numpy (the tile restatement of
tests/test_cull_certificate.py, taken over the node's triangles) and checks, on the ray families of that file -- random, secondary,
triangle soups and adversarial in-plane packets -- that

  * whenever a node certificate fires, the reference's own fp32 edge test rejects every (ray, triangle) pair of the node;
  * a node certificate never fires where a per-tile one would not: the node only closes tiles the per-tile sweep could close too, or
    tiles none of whose pairs the reference accepts (checked triangle by triangle);
  * nodes with a degenerate or non-finite triangle, or normals spread over more than ~84 degrees, are unusable;
  * node certificates are not vacuous on a height field seen from far away.
"""
import numpy as np
import pytest

from test_cull_certificate import (certificates, certified, coplanar_packet, cull_record, packet_bounds, random_packet,
                                   reference_accepts, secondary_packet)

f32 = np.float32
TILE = 10


def node_record(tris):
    """prepare_cull_kernel over a node: the tile record of the union (cull_record is written for any number of triangles)"""
    return cull_record(tris)


def bumpy_node(rng, amp, tiles):
    """`tiles` x 10 triangles of a height-field patch (5 cells per tile, tiles side by side), wound like the benchmark mesh: what a
    subtree of the k-d storage order holds"""
    cells = tiles * TILE // 2
    nx = max(1, int(round(np.sqrt(cells / 5.0))))
    while cells % nx: nx -= 1
    ny = cells // nx
    x0, y0 = rng.uniform(-18, 14), rng.uniform(-12, 2)
    cell = rng.uniform(0.05, 0.4)
    ph = rng.uniform(0, 6.28, 2)

    def z(x, y):
        return 5.0 + amp * np.sin(0.75 * x + ph[0]) * np.cos(0.5 * y + ph[1])
    tris = []
    for i in range(nx):
        for j in range(ny):
            xs, ys = x0 + i * cell, y0 + j * cell
            P = [np.array([q[0], q[1], z(*q)]) for q in ((xs, ys), (xs + cell, ys), (xs + cell, ys + cell), (xs, ys + cell))]
            tris += [[P[0], P[2], P[1]], [P[0], P[3], P[2]]]
    return np.array(tris, np.float64)


def check_node(node, o, d):
    """node certificate -> no pair accepted, triangle by triangle; and every tile of the node certified or wholly rejected too"""
    rec = node_record(node)
    pk = packet_bounds(o, d)
    if not certified(rec, pk):
        return False
    for k in range(len(node)):
        assert not reference_accepts(node[k:k + 1], o, d).any(), f"node certificate {certificates(rec, pk)} fired; triangle {k} accepted"
    return True


@pytest.mark.parametrize("tiles", [4, 16, 64])
@pytest.mark.parametrize("amp", [0.0, 0.5, 2.0])
def test_certified_nodes_are_rejected_by_the_reference_test(tiles, amp):
    rng = np.random.default_rng(100 * tiles + int(amp * 10))
    tried = fired = 0
    for it in range(60 if tiles < 64 else 25):
        node = bumpy_node(rng, amp, tiles)
        for make in (random_packet, secondary_packet, secondary_packet, coplanar_packet):
            o, d = make(rng, node)
            tried += 1
            fired += check_node(node, o, d)
    assert fired > 0.1 * tried, f"node certificates fired for {fired} of {tried} packets only"


@pytest.mark.parametrize("tiles", [4, 16])
def test_node_certificate_implies_the_tile_certificates(tiles):
    """the node's bounds contain every tile's: where the node certifies, so does (almost) every tile -- and a tile that does not is
    still rejected pair by pair by the reference (the node closes nothing the reference could accept)"""
    rng = np.random.default_rng(31 + tiles)
    node_fired = tile_checks = tile_not_certified = 0
    for it in range(60):
        node = bumpy_node(rng, rng.choice([0.0, 0.5, 2.0]), tiles)
        rec = node_record(node)
        for make in (random_packet, secondary_packet, coplanar_packet):
            o, d = make(rng, node)
            pk = packet_bounds(o, d)
            if not certified(rec, pk):
                continue
            node_fired += 1
            for t in range(tiles):
                tile = node[t * TILE:(t + 1) * TILE]
                tile_checks += 1
                if not certified(cull_record(tile), pk):
                    tile_not_certified += 1
                assert not reference_accepts(tile, o, d).any()
    assert node_fired > 0
    assert tile_not_certified <= 0.01 * tile_checks, f"{tile_not_certified} of {tile_checks} tiles of certified nodes not certified on their own"


def test_nodes_of_soups_and_degenerate_triangles():
    """a node of unrelated triangles (normals all over the sphere) is unusable; a degenerate or non-finite triangle anywhere in a node
    makes the node unusable; nearly coplanar soups stay usable and sound"""
    rng = np.random.default_rng(17)
    fired = 0
    for it in range(80):
        c = rng.uniform(-10, 10, 3)
        node = c + rng.normal(size=(4 * TILE, 3, 3)) * rng.uniform(0.1, 1.0)
        kind = it % 3
        if kind == 0:
            assert not node_record(node)["usable"]
        if kind == 1:
            node[:, :, 2] *= 1e-3                                            # nearly coplanar, wound one way: usable, tiny normal spread
            down = np.cross(node[:, 1] - node[:, 0], node[:, 2] - node[:, 0])[:, 2] < 0
            node[down] = node[down][:, ::-1]
        if kind == 2:
            node = bumpy_node(rng, 0.5, 4)
            node[7, 2] = node[7, 1]                                          # zero area
            assert not node_record(node)["usable"]
        for make in (random_packet, secondary_packet, coplanar_packet):
            o, d = make(rng, node)
            if certified(node_record(node), packet_bounds(o, d)):
                fired += 1
                assert not reference_accepts(node, o, d).any()
    assert fired > 0
    for bad_value in (np.nan, np.inf, 1e20):
        node = bumpy_node(rng, 0.5, 16)
        node[37, 1, 0] = bad_value
        rec = node_record(node)
        assert not rec["usable"] or not certified(rec, packet_bounds(*random_packet(rng, node)))


def test_in_plane_rays_of_a_far_node_are_never_certified():
    """the adversarial packet of test_cull_certificate.py against a whole node: lines within rounding noise of the plane of one of its
    triangles, passing beside it"""
    rng = np.random.default_rng(23)
    fired = 0
    for _ in range(100):
        node = bumpy_node(rng, 2.0, 16)
        o, d = coplanar_packet(rng, node, n=64, tilt=0.0)
        fired += certified(node_record(node), packet_bounds(o, d))
    assert fired == 0
