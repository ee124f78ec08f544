"""cr_update_materials and cr_update_image give device memory back, in the manner of tests/test_gpu_handle_memory.py (whose
reading of the card's free bytes, measured tolerance and repetitions are used here): a loop of growing and shrinking table
edits and whole-image edits on ONE handle ends holding what a fresh handle with the final scene holds, and cr_destroy gives
everything back.

The sizes are chosen so that a buffer kept by mistake shows: the long table is 6 MiB of f64 records (4 MiB of f32), the image
4 MiB of texels.  What a handle keeps on purpose is its update_stage, the staging buffer cr_update_primitives keeps as well
(here the image's 3 MiB of RGB8): that is why the bound is the module's tolerance plus that one buffer."""
import ctypes as C

import numpy as np
import pytest

import scenes
import shading_model as sm
from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer
from crucible_amd.scene import ImageTexture, Lambertian, RTWImage, Sphere
from test_gpu_handle_memory import MIB, SLACK, free_bytes, lost_over, settle

pytestmark = pytest.mark.gpu

LONG, IMAGE = 128 * 1024, (1024, 1024)
STAGE = IMAGE[0] * IMAGE[1] * 3


def scene():
    sc = scenes.few_spheres(4, 32, 2)
    sc.add_element(Sphere.new((0.0, 1.6, -1.0), 0.9, Lambertian.new_from_texture(ImageTexture(RTWImage(sm.seeded_image(*IMAGE, 3))), 1.0)), "globe")
    return sc, sc.flatten(), sm.camera(sc, (32, 24), 2, 6)


def tables(flat):
    short = sm.parts_of(flat)["materials"]
    long_table = (A.CrMaterial * LONG)()
    for k in range(LONG):
        long_table[k] = short[k % len(short)]
    return (A.CrMaterial * len(short))(*short), long_table


def edits(r, cam, short, long_table, images):
    """grow, render, shrink, render, repaint, render: in both precisions"""
    for k, table in enumerate((long_table, short, long_table, short)):
        r.update_materials(table)
        r.update_image(0, images[k % 2])
        for rt in (sm.F64, sm.F32):
            sm.frame(r, cam, rt)


def test_the_long_table_is_large_enough_to_show():
    assert LONG * 48 >= 6 * MIB and LONG * 32 >= 4 * MIB and IMAGE[0] * IMAGE[1] * 4 >= 4 * MIB and SLACK // 4 + STAGE < LONG * 48 + LONG * 32


def test_an_edit_loop_ends_with_a_fresh_handles_memory(hiplib):
    sc, flat, cam = scene()
    short, long_table = tables(flat)
    images = [sm.seeded_image(*IMAGE, 5), flat._image_arrays[0].copy()]
    final = sm.parts_of(flat)          # the loop ends on the short table and the uploaded texels

    def held(with_edits):
        """device bytes one handle holds with the final scene, after the loop or straight from an upload"""
        before = free_bytes()
        r = Renderer(0)
        try:
            r.upload_scene(flat if with_edits else sm.flat_of(final))
            for rt in (sm.F64, sm.F32):
                sm.frame(r, cam, rt)
            if with_edits:
                for _ in range(3):
                    edits(r, cam, short, long_table, images)
            return before - free_bytes()
        finally:
            r.close()

    held(True), held(False)            # warm-up: the runtime's own pools
    figures = [(held(True), held(False)) for _ in range(3)]
    print("bytes held after the edit loop / by a fresh handle:", figures)
    assert any(e - f <= SLACK // 4 + STAGE for e, f in figures), figures      # a long table or a second texel array kept would be 4 MiB or more above


def test_everything_comes_back(hiplib):
    sc, flat, cam = scene()
    short, long_table = tables(flat)
    images = [sm.seeded_image(*IMAGE, 5), flat._image_arrays[0].copy()]

    def cycle():
        r = Renderer(0)
        try:
            r.upload_scene(flat)
            edits(r, cam, short, long_table, images)
        finally:
            r.close()

    def bare():
        Renderer(0).close()

    settle(lambda: lost_over(cycle, 2, 8), lambda: lost_over(bare, 2, 8), "material and image edits")
