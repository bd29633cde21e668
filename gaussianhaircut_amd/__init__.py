"""gaussianhaircut_amd -- MI355X (gfx950) native strand-aligned 3D Gaussian splatting renderer + optimizer step.

One hot path of eth-ait/GaussianHaircut, rebuilt from scratch behind the reference's own Python API:

* ``gaussianhaircut_amd.diff_gaussian_rasterization``  -- ``GaussianRasterizer`` / ``GaussianRasterizationSettings``
  (reference: ``ext/diff_gaussian_rasterization_hair/diff_gaussian_rasterization/__init__.py``)
* ``gaussianhaircut_amd.gaussian_renderer``            -- ``render()`` / ``render_hair()``
  (reference: ``src/gaussian_renderer/__init__.py``)
* ``gaussianhaircut_amd.scene``                        -- ``GaussianModel`` projection helpers + Adam groups
  (reference: ``src/scene/gaussian_model.py``)
* ``gaussianhaircut_amd.between_stages`` / ``mesh``   -- the steps between the training stages: hair sphere and crop, the head-mesh
  filter, strand pruning and export (reference: ``src/preprocessing/scale_scene_into_sphere.py``,
  ``filter_flame_intersections.py``, ``export_strands.py``); point-in-mesh containment in HIP
* ``gaussianhaircut_amd.strand_prior``                 -- the strand stage's prior term between its two networks: guiding strands in
  their local frames and the latent texture, in HIP (reference: ``src/scene/gaussian_model_strands.py:456-515``)
* ``gaussianhaircut_amd.strand_view``                  -- a preview of the groom: strands as depth-tested polylines over the head
  mesh, shaded, along an interpolated camera path, in HIP (reference: ``src/postprocessing/render_video.py``, without Blender)
* ``gaussianhaircut_amd.comparison``                   -- the comparison video's frames: strand render over white, Pillow-exact resizes,
  crop and the three-panel strip, in HIP (reference: ``src/postprocessing/concat_video.py``, without ffmpeg)
* ``gaussianhaircut_amd.parallel``                    -- view-sharded data parallel step (RCCL all-reduce of Gaussian grads)

The compute lives in ``csrc/`` (hand-written HIP, C ABI in ``include/ghr.h``).  No CPU fallback exists.
"""
__version__ = "0.1.0"
