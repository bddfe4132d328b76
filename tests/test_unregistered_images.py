"""An unregistered image in the Python object model is an `Image` with `registered = False`; an image without the attribute is registered, so nothing
changes for the reconstructions that never heard of the flag.  The places that used to treat every image as registered:
`Reconstruction.RegImageIds` and, through it, `Normalize(use_images=True)`, `GlobalBundleAdjustmentConfig` and the per-camera count of
`LocalBundleAdjustmentConfig`; `IncrementalTriangulator.flatten` hands the flag to the device.  Host only."""
import numpy as np

import incremental_registration_scene as irs
from privacy_preserving_sfm_amd import synthetic
from privacy_preserving_sfm_amd.bundle_adjustment import GlobalBundleAdjustmentConfig, IncrementalMapperOptions, LocalBundleAdjustmentConfig
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator


def test_without_the_attribute_every_image_is_registered_in_id_order():
    rec, graph, _ = irs.make_world(seed=0)
    for im in rec.images.values():
        del im.registered
    assert rec.RegImageIds() == list(range(irs.NUM_IMAGES))
    assert IncrementalTriangulator(graph, rec).flatten()[0]["image_registered"].tolist() == [1] * irs.NUM_IMAGES


def test_reg_image_ids_honours_the_flag_and_the_order_of_registration():
    rec, graph, _ = irs.make_world(seed=0)
    assert rec.RegImageIds() == [0, 1, 2]
    assert IncrementalTriangulator(graph, rec).flatten()[0]["image_registered"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    rec.images[6].registered, rec.images[6].reg_index = True, 0      # registered first ...
    rec.images[4].registered, rec.images[4].reg_index = True, 1      # ... and second
    assert rec.RegImageIds() == [0, 1, 2, 6, 4]
    config = GlobalBundleAdjustmentConfig(rec)
    assert sorted(config.Images()) == [0, 1, 2, 4, 6] and config.HasConstantPose(0) and config.HasConstantTvec(1)
    for i in (0, 1, 2):
        rec.images[i].registered = False
    config = GlobalBundleAdjustmentConfig(rec)      # the gauge sits on the first two REGISTERED images
    assert sorted(config.Images()) == [4, 6] and config.HasConstantPose(6) and config.HasConstantTvec(4)


def test_normalize_moves_registered_images_only():
    rec, graph, info = irs.make_world(seed=0)
    before = {i: rec.images[i].tvec.copy() for i in rec.images}
    rec.Normalize()
    assert all(not np.array_equal(before[i], rec.images[i].tvec) for i in (0, 1, 2))
    assert all(np.array_equal(before[i], rec.images[i].tvec) for i in range(3, irs.NUM_IMAGES))      # as the reference: registered images only
    # the robust box is taken over the three registered centres, not over the identity poses of the others
    centres = np.array([-synthetic.quat_to_rot(rec.images[i].qvec).T @ rec.images[i].tvec for i in (0, 1, 2)])
    assert abs(np.linalg.norm(centres.max(axis=0) - centres.min(axis=0)) - 10.0) < 1e-5      # (the box is measured on floats)


def test_local_config_counts_registered_images_per_camera():
    rec, graph, _ = irs.make_world(seed=0)
    options = IncrementalMapperOptions()
    config, _ = LocalBundleAdjustmentConfig(rec, options, 0, [1, 2], [])
    assert not config.IsConstantCamera(0)      # all three registered images of camera 0 are in the bundle: the five unregistered ones do not count
    config, _ = LocalBundleAdjustmentConfig(rec, options, 0, [1], [])
    assert config.IsConstantCamera(0)
