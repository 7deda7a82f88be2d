"""Scene-layout wrapper around the DDPM -- drop-in for
scene_synthesis/networks/diffusion_scene_layout_ddpm.py (``DiffusionSceneLayout_DDPM``, ``train_on_batch``,
``validate_on_batch``): same constructor, config keys, sample_params keys, method names, state_dict keys
(``diffusion.model.*``, ``positional_embedding``, ``fc_text_f.*``, ``fc_arrange_condition.*`` ...).

What changed underneath:
* the instance embedding is broadcast over the batch as a stride-0 view instead of a gathered (B,N,128)
  copy (:174-175), which lets the denoiser push N instead of B*N rows through its 9 context MLPs;
* ``train_on_batch`` reads all logged scalars with ONE device->host copy instead of 11 ``.item()`` syncs
  (:461-473), and all-reduces gradients over RCCL when torch.distributed is initialised (data parallel);
* post-filtering of empty boxes (:351-406) is vectorised; it still looks only at batch row 0, as the reference.
Optional third-party encoders (BERT / CLIP) are imported only when the config asks for them; the floor-plan encoder of a
``room_mask_condition`` model is the package's own (feature_extractors.py): ``room_mask`` is then (B, c, H, W) or (1, c, H, W) -- one
room for all B layouts, encoded once per call, outside every captured loop -- and the same mask serves ``wall_scale``.
"""
import torch
import torch.nn as nn
from torch.nn import Module

from ..stats_logger import StatsLogger
from .denoise_net import Unet1D
from .diffusion_ddpm import DiffusionPoint


class _TwoLayer(nn.Sequential):
    """Linear(bias=False) -> LeakyReLU(0.1) -> Linear(bias=False): the instance / partial / arrange condition MLPs of the
    reference (:94-125).  Same parameters and state_dict keys (``0.weight``, ``2.weight``) as the reference's nn.Sequential;
    forward and backward run on the fp32 MFMA GEMM and the elementwise HIP kernels (autograd_ops), not on ATen / rocBLAS."""

    def __init__(self, n_in, n_out):
        super().__init__(nn.Linear(n_in, n_out, bias=False), nn.LeakyReLU(0.1, inplace=True),
                         nn.Linear(n_out, n_out, bias=False))

    def forward(self, x):
        from .._lib import ACT_LEAKY01
        from ..autograd_ops import ActFn, linear_any
        h = linear_any(x, self[0].weight)
        h = ActFn.apply(h.reshape(-1, h.shape[-1]).contiguous(), ACT_LEAKY01).reshape(h.shape)
        return linear_any(h, self[2].weight)


class _HipLinear(nn.Linear):
    """nn.Linear whose forward / backward run on the HIP GEMM (fc_text_f, fc_room_f)."""

    def forward(self, x):
        from ..autograd_ops import linear_any
        return linear_any(x, self.weight, self.bias)


def _two_layer(n_in, n_out):
    return _TwoLayer(n_in, n_out)


class DiffusionSceneLayout_DDPM(Module):
    # The reference's call sites pass ``batch_seeds=torch.arange(i, i + 1)`` for scene i and its sample() never reads it; this drop-in
    # ignores it too (the seeded-parity contract rests on that) unless a caller opts in: True makes a non-None ``batch_seeds`` the
    # ``scene_seeds`` of that call, so the unchanged scripts produce, scene by scene, what generate_layout_batched(scene_seeds=range(n)) does.
    honour_batch_seeds = False

    def __init__(self, n_classes, feature_extractor, config):
        super().__init__()
        self.room_mask_condition = config.get("room_mask_condition", True)
        self.text_condition = config.get("text_condition", False)
        self.text_glove_embedding = config.get("text_glove_embedding", False)
        self.text_clip_embedding = config.get("text_clip_embedding", False)
        if self.room_mask_condition:
            self.feature_extractor = feature_extractor
            self.fc_room_f = _HipLinear(self.feature_extractor.feature_size, config["latent_dim"])
            print('use room mask as condition')
        elif self.text_condition:
            text_embed_dim = config.get("text_embed_dim", 512)
            if self.text_glove_embedding:
                self.fc_text_f = _HipLinear(50, text_embed_dim)
                print('use text as condition, and pretrained glove embedding')
            elif self.text_clip_embedding:
                import clip
                device = "cuda" if torch.cuda.is_available() else "cpu"
                self.clip_model, self.clip_preprocess = clip.load("ViT-B/32", device=device)
                for p in self.clip_model.parameters():
                    p.requires_grad = False
                print('use text as condition, and pretrained clip embedding')
            else:
                # ``text_bert_cached: true`` (new key, default false = reference behaviour): the frozen BERT encoder is not
                # instantiated; batches carry its cached last_hidden_state as ``desc_bert`` (B, L, 768), produced once
                # per description by diffuscene_amd.text_cache.BertFeatureCache
                self.text_bert_cached = config.get("text_bert_cached", False)
                if not self.text_bert_cached:
                    from transformers import BertModel, BertTokenizer
                    self.tokenizer = BertTokenizer.from_pretrained('bert-base-cased')
                    self.bertmodel = BertModel.from_pretrained("bert-base-cased")
                    for p in self.bertmodel.parameters():
                        p.requires_grad = False
                self.fc_text_f = _HipLinear(768, text_embed_dim)
                print('use text as condition, and pretrained bert model')
        else:
            print('NOT use room and text as condition')

        if config["net_type"] == "unet1d":
            denoise_net = Unet1D(**config["net_kwargs"])
        else:
            raise NotImplementedError()
        self.diffusion = DiffusionPoint(denoise_net=denoise_net, config=config, **config["diffusion_kwargs"])
        # ``text_drop_prob`` (new key, default 0.0 = reference behaviour): in training mode every scene's text features are replaced by
        # the null condition (zeros after fc_text_f) with this probability -- what classifier-free guidance (``guidance_scale``) needs
        self.text_drop_prob = float(config.get("text_drop_prob", 0.0))
        if not 0.0 <= self.text_drop_prob <= 1.0:
            raise ValueError("text_drop_prob must lie in [0, 1], got %r" % (config.get("text_drop_prob"),))
        self.n_classes = n_classes
        self.config = config

        self.objectness_dim = config.get("objectness_dim", 1)
        self.class_dim = config.get("class_dim", 21)
        self.translation_dim = config.get("translation_dim", 3)
        self.size_dim = config.get("size_dim", 3)
        self.angle_dim = config.get("angle_dim", 1)
        self.bbox_dim = self.translation_dim + self.size_dim + self.angle_dim
        self.objfeat_dim = config.get("objfeat_dim", 0)

        self.learnable_embedding = config.get("learnable_embedding", False)
        self.instance_condition = config.get("instance_condition", False)
        self.sample_num_points = config.get("sample_num_points", 12)
        self.instance_emb_dim = config.get("instance_emb_dim", 64)
        if self.learnable_embedding:
            if self.instance_condition:
                self.register_parameter("positional_embedding",
                                        nn.Parameter(torch.randn(self.sample_num_points, self.instance_emb_dim)))
            else:
                self.instance_emb_dim = 0
        else:
            if self.instance_condition:
                self.fc_instance_condition = _two_layer(self.sample_num_points, self.instance_emb_dim)
            else:
                self.instance_emb_dim = 0

        self.room_partial_condition = config.get("room_partial_condition", False)
        self.partial_num_points = config.get("partial_num_points", 0)
        self.partial_emb_dim = config.get("partial_emb_dim", 64)
        full = self.bbox_dim + self.class_dim + self.objectness_dim + self.objfeat_dim
        if self.room_partial_condition:
            self.fc_partial_condition = _two_layer(full, self.partial_emb_dim)
        else:
            self.partial_emb_dim = 0
        self.room_arrange_condition = config.get("room_arrange_condition", False)
        self.arrange_emb_dim = config.get("arrange_emb_dim", 64)
        if self.room_arrange_condition:
            self.fc_arrange_condition = _two_layer(full - self.translation_dim - self.angle_dim, self.arrange_emb_dim)
        else:
            self.arrange_emb_dim = 0

    # ------------------------------------------------------------------------------------ conditions
    def _instance_condition(self, batch_size, device):
        if not self.instance_condition:
            return None
        if self.learnable_embedding:
            # same values as positional_embedding[arange(N)].repeat(B, 1, 1) (:174-175), without the copy
            return self.positional_embedding[None, :, :].expand(batch_size, -1, -1)
        eye = torch.eye(self.sample_num_points, device=device)
        return self.fc_instance_condition(eye)[None].expand(batch_size, -1, -1)

    def _base_condition(self, room_mask, batch_size, num_points, device):
        room_layout_f = self.fc_room_f(self.feature_extractor(room_mask)) if self.room_mask_condition else None
        if room_layout_f is not None and room_layout_f.shape[0] == 1 and batch_size > 1:
            room_layout_f = room_layout_f.expand(batch_size, -1)       # one room, B layouts: encoded once
        inst = self._instance_condition(batch_size, device)
        if room_layout_f is not None and inst is not None:
            return torch.cat([room_layout_f[:, None, :].repeat(1, num_points, 1), inst], dim=-1).contiguous()
        if room_layout_f is not None:
            return room_layout_f[:, None, :].repeat(1, num_points, 1)
        return inst

    def attach_bert_cache(self, cache):
        """Use a text_cache.BertFeatureCache for the descriptions instead of running BERT inside every step."""
        object.__setattr__(self, "_bert_cache", cache)

    def _text_condition(self, text, desc_emb, device, desc_bert=None):
        if not self.text_condition:
            return None
        if self.text_glove_embedding:
            return self.fc_text_f(desc_emb)
        if self.text_clip_embedding:
            import clip
            return self.clip_model.encode_text(clip.tokenize(text).to(device))
        cache = getattr(self, "_bert_cache", None)
        if desc_bert is None and cache is not None:
            desc_bert = cache.batch(text, device)                # frozen encoder: features are a function of the text only
        if desc_bert is not None:
            return self.fc_text_f(desc_bert)
        if getattr(self, "text_bert_cached", False):
            raise KeyError("text_bert_cached: the batch must carry 'desc_bert' (B, L, 768) or a BertFeatureCache must be "
                           "attached (attach_bert_cache)")
        tokenized = self.tokenizer(text, return_tensors='pt', padding=True).to(device)
        return self.fc_text_f(self.bertmodel(**tokenized).last_hidden_state)

    def _arrange_input(self, boxes):
        tr, sz, bb = self.translation_dim, self.size_dim, self.bbox_dim
        return torch.cat([boxes[:, :, tr:tr + sz], boxes[:, :, bb:]], dim=-1).contiguous()

    def _check_room(self, room_mask, batch_size, what="sample"):
        """The refusal of a floor-plan-conditioned model's ``room_mask``, before anything is computed or drawn: (batch_size, c, H, W), or
        (1, c, H, W) -- one room for all ``batch_size`` layouts, encoded once and expanded.  Other models take the mask as they did."""
        if not self.room_mask_condition:
            return
        if not isinstance(room_mask, torch.Tensor) or room_mask.dim() != 4:
            raise ValueError("%s: room_mask must be a (B, c, H, W) tensor on a room_mask_condition model, got %s"
                             % (what, tuple(room_mask.shape) if isinstance(room_mask, torch.Tensor) else type(room_mask).__name__))
        if room_mask.shape[0] not in (1, int(batch_size)):
            raise ValueError("%s: room_mask holds %d rooms for a batch of %d (give one room per scene, or one room for all)"
                             % (what, room_mask.shape[0], batch_size))

    def _sampling_conditions(self, room_mask, num_points, device, text=None, padded_partial=None, input_boxes=None, batch_size=None):
        """(condition, condition_cross) of a sampling call, reference :233-262: the base condition, then the embedding of the given
        objects padded with zeros to ``num_points`` (room_partial_condition) and of the kept channels of ``input_boxes``
        (room_arrange_condition), and the text features.  One copy for ``sample`` and the batched / strided entry points.  The floor-plan
        features of a room_mask_condition model are computed here, once per call and outside every captured loop; ``batch_size`` is the
        number of scenes they are expanded to when the mask holds one room."""
        if not self.room_mask_condition or batch_size is None:
            batch_size = room_mask.size(0)
        condition = self._base_condition(room_mask, batch_size, num_points, device)
        if self.room_partial_condition:
            condition = torch.cat([condition, self.fc_partial_condition(padded_partial)], dim=-1).contiguous()
        if self.room_arrange_condition:
            condition = torch.cat([condition, self.fc_arrange_condition(self._arrange_input(input_boxes))],
                                  dim=-1).contiguous()
        return condition, self._text_condition(text, text, device)

    # ------------------------------------------------------------------------------------ training
    def get_loss(self, sample_params):
        """reference :131-226"""
        target, condition, condition_cross = self._loss_inputs(sample_params)
        return self.diffusion.get_loss_iter(target, condition=condition, condition_cross=condition_cross)

    def _loss_inputs(self, sample_params):
        """The part of get_loss before the diffusion call (:131-221): diffusion target (B, N, C), per-object condition and
        cross-attention condition."""
        class_labels = sample_params["class_labels"]
        translations, sizes, angles = sample_params["translations"], sample_params["sizes"], sample_params["angles"]
        batch_size, num_points, _ = class_labels.shape
        device = class_labels.device
        full = self.bbox_dim + self.class_dim + self.objectness_dim + self.objfeat_dim
        packed = sample_params.get("_packed")      # diffuscene_amd.datasets batches arrive already in channel order
        if (self.config["point_dim"] == full and packed is not None and packed.shape[-1] == full
                and self.objectness_dim == 0 and packed.is_contiguous()):
            target = packed
        elif self.config["point_dim"] == full:
            parts = [translations, sizes, angles, class_labels]
            if self.objectness_dim > 0:
                parts.append(sample_params["objectness"])
            if self.objfeat_dim > 0:
                parts.append(sample_params["objfeats_32"] if self.objfeat_dim == 32 else sample_params["objfeats"])
            target = torch.cat(parts, dim=-1).contiguous()
        elif self.config["point_dim"] == self.bbox_dim:
            target = torch.cat([translations, sizes, angles], dim=-1).contiguous()
        else:
            raise NotImplementedError
        condition = self._base_condition(sample_params["room_layout"] if self.room_mask_condition else None,
                                         batch_size, num_points, device)
        if self.room_partial_condition:
            mask = torch.zeros((batch_size, num_points, 1), device=device)
            mask[:, :self.partial_num_points] = 1.0
            condition = torch.cat([condition, self.fc_partial_condition(target * mask)], dim=-1).contiguous()
        if self.room_arrange_condition:
            condition = torch.cat([condition, self.fc_arrange_condition(self._arrange_input(target))],
                                  dim=-1).contiguous()
            tr, sz, bb = self.translation_dim, self.size_dim, self.bbox_dim
            target = torch.cat([target[:, :, 0:tr], target[:, :, tr + sz:bb]], dim=-1).contiguous()
        condition_cross = self._text_condition(sample_params.get("description"), sample_params.get("desc_emb"), device,
                                               desc_bert=sample_params.get("desc_bert"))
        keep = self._text_keep(sample_params, batch_size, device) if condition_cross is not None else None
        if keep is not None:
            condition_cross = self._gate_text(condition_cross, keep)
        return target, condition, condition_cross

    def _text_keep(self, sample_params, batch_size, device):
        """The (B,) bool keep mask of the text-condition dropout, or None when nothing is dropped.  ``sample_params["_cond_keep"]``
        overrides the draw (goldens); otherwise, with text_drop_prob = p > 0 in training mode, ONE draw u = torch.rand((B,)) is made --
        after the text features, before the t and noise draws of the loss -- and keep = u >= p.  p == 0 or eval mode: no draw."""
        keep = sample_params.get("_cond_keep")
        if keep is not None:
            keep = torch.as_tensor(keep)
            if keep.dtype != torch.bool or tuple(keep.shape) != (batch_size,):
                raise ValueError("_cond_keep must be a (%d,) bool tensor, got %s %s" % (batch_size, tuple(keep.shape), keep.dtype))
            return keep.to(device)
        p = getattr(self, "text_drop_prob", 0.0)
        if p > 0.0 and self.training:
            return torch.rand((batch_size,), device=device) >= p
        return None

    def _gate_text(self, condition_cross, keep):
        """Rows of the dropped scenes replaced by zeros -- a select (dsc_scene_gate_f32), forward and on the gradient: a dropped scene
        neither reads nor propagates its features."""
        from ..autograd_ops import SceneGateFn
        return SceneGateFn.apply(condition_cross, keep)

    # ------------------------------------------------------------------------------------ sampling
    def _seeded(self, scene_seeds, batch_seeds, batch_size, device):
        """The noise keyword of a loop call: none at all without seeds -- that call stays what it was --, else a SceneNoise over the
        checked seeds (ops.scene_seeds: ValueError before anything is drawn).  ``scene_seeds``: one int in [0, 2**63) per scene; scene
        b of the call is then a function of its seed, its own inputs, the model and the loop kind -- not of the batch size, its
        position, the other scenes or earlier calls (up to the GEMM dispatch of that batch size) --, the device
        generator is left untouched, and repeated seeds give identical scenes."""
        if scene_seeds is None and self.honour_batch_seeds:
            scene_seeds = batch_seeds
        if scene_seeds is None:
            return {}
        from .. import ops
        from ..scene_noise import SceneNoise
        return dict(noise_fn=SceneNoise(ops.scene_seeds(scene_seeds, batch_size, device), device))

    def sample(self, room_mask, num_points, point_dim, batch_size=1, text=None, partial_boxes=None,
               input_boxes=None, ret_traj=False, ddim=False, clip_denoised=False, freq=40, batch_seeds=None,
               sampling_timesteps=None, ddim_sampling_eta=0.0, guidance_scale=None, scene_seeds=None, collision_scale=None,
               collision_steps=None, sampling_solver=None,
               wall_scale=None, wall_steps=None, room_side=None):
        """reference :228-310.  ``ddim`` keeps the reference's meaning: accepted and ignored.  ``sampling_timesteps`` is the DDIM
        switch: None runs the T-step DDPM loop; an integer S runs ``gen_samples_ddim`` (S strided steps, ``ddim_sampling_eta``) for
        unconditional, instance- and text-conditioned generation, and with ``ret_traj`` returns its S + 1 states.  The reference
        defines no strided completion or re-arrangement, so this drop-in method refuses the combination; strided inpainting lives on
        the scene-level entry points (``complete_scene_batched``, ``arrange_scene_batched``, ``complete_scene``, ``arrange_scene`` with
        ``sampling_timesteps``), over ``complete_samples_ragged_ddim`` / ``arrange_samples_ddim``.
        ``guidance_scale`` (None: the plain conditional model, this method as it was): a float or ``batch_size`` per-scene values w, the
        classifier-free guidance scale of a text-conditioned model -- every step uses u + w (c - u), c the denoiser on the text features
        and u the denoiser on the null condition (condition_cross == 0) (``gen_samples_guided`` / ``gen_samples_guided_ddim`` with
        ``sampling_timesteps``).  Generation only; needs ``text``.
        ``scene_seeds`` (None: the device generator, this method as it was): one seed per scene, see ``_seeded``; combines with every
        other keyword.  ``batch_seeds`` stays accepted and ignored (``honour_batch_seeds``).
        ``collision_scale`` (None: this method as it was): a float or ``batch_size`` per-scene weights w >= 0 of collision steering --
        after every model call whose timestep is below ``collision_steps`` (None: every step; an integer K: the last K timesteps) the
        clamped x0 estimate of scene b moves by -w[b] * dE/d(translations), E the summed pairwise IoU of its non-empty boxes
        (GaussianDiffusion._steer_inputs).  Generation and completion, T-step and strided, guided or not, seeded or
        not; re-arrangement and ``ret_traj`` refuse it.  Needs the train-stats file for the de-normalisation bounds.
        ``sampling_solver`` (None: this method as it was; "dpmpp_2m"): the multistep DPM-Solver++(2M) on the strided loop -- the S
        steps are taken on the extrapolated x0 estimate D = x0 + e_k (x0 - x0_prev) (``_check_solver``), one model
        call per step as before; combines with guidance, steering and seeds.  Needs ``sampling_timesteps`` and
        ``ddim_sampling_eta == 0``.
        ``wall_scale`` (None: this method as it was): a float or ``batch_size`` per-scene weights w >= 0 of floor-plan steering -- after
        every model call whose timestep is below ``wall_steps`` (None: every step) the clamped x0 estimate of scene b moves by
        -w[b] * dE/d(x, z translations), E the out-of-room energy of the oriented footprints of its non-empty boxes over the distance
        field of ``room_mask`` ((B, 1, H, W) or (1, 1, H, W), inside > 0.5), rendered in the window [-room_side, room_side]^2 metres
        (``_check_walls``, GaussianDiffusion._wall_inputs).  Runs after collision steering; the same loops accept and
        refuse it.  Needs ``room_side`` and the train-stats file."""
        self._check_room(room_mask, batch_size)
        if guidance_scale is not None:
            self._check_guidance(text, partial_boxes, input_boxes, ret_traj)
        steer = self._check_steering(collision_scale, collision_steps, wall_scale, wall_steps, room_side, room_mask,
                                     (batch_size, num_points, point_dim), input_boxes, ret_traj)
        solver = self._check_solver(sampling_solver, sampling_timesteps, ddim_sampling_eta)
        if sampling_timesteps is not None and (partial_boxes is not None or input_boxes is not None):
            raise NotImplementedError("sampling_timesteps (DDIM) is defined for generation only: scene completion and "
                                      "re-arrangement run the full DDPM loop (call them with sampling_timesteps=None)")
        device = room_mask.device
        seeded = self._seeded(scene_seeds, batch_seeds, batch_size, device)
        noise = torch.randn((batch_size, num_points, point_dim))   # CPU draw kept: it advances the CPU RNG (:232)
        padded = None
        if self.room_partial_condition:
            zeros = torch.zeros((batch_size, num_points - partial_boxes.shape[1], partial_boxes.shape[2]),
                                device=device)
            padded = torch.cat([partial_boxes, zeros], dim=1).contiguous()
        condition, condition_cross = self._sampling_conditions(room_mask, num_points, device, text=text, padded_partial=padded,
                                                               input_boxes=input_boxes, batch_size=batch_size)
        if self.text_condition and not (self.text_glove_embedding or self.text_clip_embedding):
            print('after bert:', condition_cross.shape)
        if input_boxes is not None:
            print('scene arrangement sampling')
            return self.diffusion.arrange_samples(noise.shape, device, condition=condition,
                                                  condition_cross=condition_cross, clip_denoised=clip_denoised,
                                                  input_boxes=input_boxes, **seeded)
        if partial_boxes is not None:
            print('scene completion sampling')
            return self.diffusion.complete_samples(noise.shape, device, condition=condition,
                                                   condition_cross=condition_cross, clip_denoised=clip_denoised,
                                                   partial_boxes=partial_boxes, **seeded, **steer)
        print('unconditional / conditional generation sampling')
        if guidance_scale is not None:
            if condition_cross is None or condition_cross.dim() != 3:
                raise ValueError("guidance_scale: the text encoder must give (B, L, text_embed_dim) features, got %s (the null "
                                 "condition is defined on the cross-attention features)"
                                 % (None if condition_cross is None else tuple(condition_cross.shape),))
            from .. import ops
            scale = ops.guidance_scales(guidance_scale, batch_size, "cpu")     # checked on the host; the loop uploads it
            if sampling_timesteps is not None:
                return self.diffusion.gen_samples_guided_ddim(noise.shape, device, condition=condition, condition_cross=condition_cross,
                                                              guidance_scale=scale, sampling_timesteps=sampling_timesteps,
                                                              ddim_sampling_eta=ddim_sampling_eta, **seeded, **steer, **solver)
            return self.diffusion.gen_samples_guided(noise.shape, device, condition=condition, condition_cross=condition_cross,
                                                     guidance_scale=scale, clip_denoised=clip_denoised, **seeded, **steer)
        if sampling_timesteps is not None:
            return self.diffusion.gen_samples_ddim(noise.shape, device, condition=condition, condition_cross=condition_cross,
                                                   clip_denoised=clip_denoised, sampling_timesteps=sampling_timesteps,
                                                   ddim_sampling_eta=ddim_sampling_eta, return_all_timesteps=bool(ret_traj), **seeded,
                                                   **steer, **solver)
        if ret_traj:
            return self.diffusion.gen_sample_traj(noise.shape, device, freq=freq, condition=condition,
                                                  condition_cross=condition_cross, clip_denoised=clip_denoised, **seeded)
        return self.diffusion.gen_samples(noise.shape, device, condition=condition, condition_cross=condition_cross,
                                          clip_denoised=clip_denoised, **seeded, **steer)

    def _check_steering(self, collision_scale, collision_steps, wall_scale, wall_steps, room_side, room_mask, shape, input_boxes=None,
                        ret_traj=False, what="sample"):
        """_check_steer and _check_walls -> the steering keywords the loop receives."""
        steer = self._check_steer(collision_scale, collision_steps, shape, input_boxes, ret_traj, what)
        steer.update(self._check_walls(wall_scale, wall_steps, room_side, room_mask, shape, input_boxes, ret_traj, what))
        return steer

    def _refuse_steering(self, keyword, input_boxes, ret_traj):
        """Where no steering term applies: re-arrangement and trajectories."""
        if input_boxes is not None or self.room_arrange_condition:
            raise ValueError("%s: re-arrangement diffuses [translation | angle] only, the boxes are not steered there" % keyword)
        if ret_traj:
            raise ValueError("%s: the steered loops return the final scenes only (ret_traj is not supported)" % keyword)

    def _check_steer(self, collision_scale, collision_steps, shape, input_boxes=None, ret_traj=False, what="sample"):
        """The refusals of ``collision_scale`` / ``collision_steps``, before anything is computed or drawn -> the keywords the loop
        receives: none at all without steering, so that call stays what it was."""
        if collision_scale is None and collision_steps is None:
            return {}
        self._refuse_steering("collision_scale", input_boxes, ret_traj)
        self.diffusion.diffusion._steer_inputs(tuple(int(v) for v in shape), "cpu", collision_scale, collision_steps, what)
        return dict(collision_scale=collision_scale, collision_steps=collision_steps)

    def _check_walls(self, wall_scale, wall_steps, room_side, room_mask, shape, input_boxes=None, ret_traj=False, what="sample"):
        """The refusals of ``wall_scale`` / ``wall_steps`` / ``room_side``, before anything is computed or drawn -> the keywords the loop
        receives (the room mask among them): none at all without floor-plan steering, so that call stays what it was."""
        if wall_scale is None and wall_steps is None and room_side is None:
            return {}
        self._refuse_steering("wall_scale", input_boxes, ret_traj)
        self.diffusion.diffusion._wall_inputs(tuple(int(v) for v in shape), "cpu", wall_scale, wall_steps, room_side, room_mask, what,
                                              field=False)
        return dict(wall_scale=wall_scale, wall_steps=wall_steps, room_side=room_side, room_mask=room_mask)

    def _check_solver(self, sampling_solver, sampling_timesteps, ddim_sampling_eta, what="sample"):
        """The refusals of ``sampling_solver``, before anything is computed or drawn -- an unknown name, no ``sampling_timesteps``,
        ``ddim_sampling_eta != 0`` -> the keyword the strided loop receives: none at all without a solver, so that call stays what it
        was."""
        if sampling_solver is None:
            return {}
        from .diffusion_ddpm import _check_solver
        strided = None if sampling_timesteps is None else self._check_strided(sampling_timesteps, ddim_sampling_eta)
        return dict(sampling_solver=_check_solver(sampling_solver, strided, what))

    def _check_resample(self, resample, resample_steps, sampling_solver=None, ret_traj=False, what="sample"):
        """The refusals of ``resample`` / ``resample_steps``, before anything is computed or drawn -- not a pair of integers >= 1, K
        without the pair or outside [0, T], a multistep solver, ``ret_traj``, a room_partial_condition / room_arrange_condition model
        -> the keywords the loop receives: none at all without resampling, so that call stays what it was."""
        if resample is None and resample_steps is None:
            return {}
        from .. import ops
        if resample is None:
            raise ValueError("%s: resample_steps goes with resample=(jump_length, n_resample)" % what)
        ops.resample_pair(resample, what)
        ops.resample_steps_value(resample_steps, int(self.config["diffusion_kwargs"].get("time_num", 1000)), what)
        if sampling_solver is not None:
            raise ValueError("%s: resample does not combine with sampling_solver=%r: the x0 history is void after a jump"
                             % (what, sampling_solver))
        if ret_traj:
            raise ValueError("%s: resample returns the final scenes only (ret_traj is not supported)" % what)
        if self.room_partial_condition or self.room_arrange_condition:
            raise ValueError("%s: resample on a room_partial_condition / room_arrange_condition model: its condition tensors already "
                             "encode a prefix / a sub-shape of the scene" % what)
        return dict(resample=resample, resample_steps=resample_steps)

    def _check_guidance(self, text, partial_boxes=None, input_boxes=None, ret_traj=False):
        """The refusals of ``guidance_scale``, before anything is computed or drawn."""
        if not self.text_condition:
            raise ValueError("guidance_scale needs a text-conditioned model (text_condition: true): guidance contrasts the text "
                             "condition with the null condition")
        if text is None:
            raise ValueError("guidance_scale needs text=...: there is nothing to guide towards without a prompt")
        if partial_boxes is not None or input_boxes is not None:
            raise ValueError("guidance_scale is defined for generation only, not for completion or re-arrangement")
        if ret_traj:
            raise ValueError("guidance_scale: the guided loops return the final scenes only (ret_traj is not supported)")

    @torch.no_grad()
    def generate_layout(self, room_mask, num_points, point_dim, batch_size=1, text=None, ret_traj=False, ddim=False,
                        clip_denoised=False, batch_seeds=None, device="cpu", keep_empty=False, sampling_timesteps=None,
                        ddim_sampling_eta=0.0, guidance_scale=None, scene_seeds=None, collision_scale=None, collision_steps=None,
                        sampling_solver=None,
                        wall_scale=None, wall_steps=None, room_side=None):
        samples = self.sample(room_mask, num_points, point_dim, batch_size, text=text, ret_traj=ret_traj, ddim=ddim,
                              clip_denoised=clip_denoised, batch_seeds=batch_seeds, **_ddim_kwargs(sampling_timesteps, ddim_sampling_eta),
                              **_guidance_kwargs(guidance_scale), **_seed_kwargs(scene_seeds),
                              **_steer_kwargs(collision_scale, collision_steps),
                              **_wall_kwargs(wall_scale, wall_steps, room_side), **_solver_kwargs(sampling_solver))
        return self.delete_empty_from_network_samples(samples, device=device, keep_empty=keep_empty)

    @torch.no_grad()
    def generate_layout_progressive(self, room_mask, num_points, point_dim, batch_size=1, text=None, ret_traj=False,
                                    ddim=False, clip_denoised=False, batch_seeds=None, device="cpu", keep_empty=False,
                                    num_step=100, guidance_scale=None, scene_seeds=None):
        """``guidance_scale``: the guided loops keep no trajectory, so the guided call returns the final scenes under the key of the
        last step, ``{0: dict}``."""
        if guidance_scale is not None:
            self._check_guidance(text)
            samples = self.sample(room_mask, num_points, point_dim, batch_size, text=text, ddim=ddim, clip_denoised=clip_denoised,
                                  batch_seeds=batch_seeds, guidance_scale=guidance_scale, **_seed_kwargs(scene_seeds))
            return {0: self.delete_empty_from_network_samples(samples, device=device, keep_empty=keep_empty)}
        traj = self.sample(room_mask, num_points, point_dim, batch_size, text=text, ret_traj=ret_traj, ddim=ddim,
                           clip_denoised=clip_denoised, batch_seeds=batch_seeds, freq=num_step, **_seed_kwargs(scene_seeds))[1:]
        return {num_step * i: self.delete_empty_from_network_samples(s, device=device, keep_empty=keep_empty)
                for i, s in enumerate(traj)}

    def _check_strided(self, sampling_timesteps, ddim_sampling_eta):
        """(S, eta) of a strided call, ValueError before any loop runs."""
        from .diffusion_ddpm import _check_ddim
        return _check_ddim(int(self.config["diffusion_kwargs"].get("time_num", 1000)), sampling_timesteps, ddim_sampling_eta)

    def _complete_strided(self, room_mask, num_points, point_dim, padded, counts, batch_size, sampling_timesteps, ddim_sampling_eta,
                          seeded={}, steer={}, solver={}, resample={}):
        """The strided completion call behind complete_scene / complete_scene_batched: the condition assembly of ``sample`` (the CPU
        draw included), then ``complete_samples_ragged_ddim``."""
        device = room_mask.device
        torch.randn((batch_size, num_points, point_dim))           # CPU draw kept, as in sample (:232)
        if self.room_arrange_condition:
            raise ValueError("scene completion: a room_arrange_condition model re-arranges scenes (arrange_scene_batched)")
        condition, condition_cross = self._sampling_conditions(room_mask, num_points, device, padded_partial=padded, batch_size=batch_size)
        print('scene completion sampling')
        return self.diffusion.complete_samples_ragged_ddim((batch_size, num_points, point_dim), device, condition=condition,
                                                           condition_cross=condition_cross, partial_boxes=padded, num_partial=counts,
                                                           sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta,
                                                           **seeded, **steer, **solver, **resample)

    def _arrange_strided(self, room_mask, num_points, point_dim, input_boxes, batch_size, sampling_timesteps, ddim_sampling_eta,
                         seeded={}, solver={}):
        """The strided re-arrangement call behind arrange_scene / arrange_scene_batched: the condition assembly of ``sample`` (the CPU
        draw included), then ``arrange_samples_ddim``."""
        device = room_mask.device
        torch.randn((batch_size, num_points, point_dim))           # CPU draw kept, as in sample (:232)
        if self.room_partial_condition:
            raise ValueError("re-arrangement: a room_partial_condition model completes scenes (complete_scene_batched)")
        condition, condition_cross = self._sampling_conditions(room_mask, num_points, device, input_boxes=input_boxes, batch_size=batch_size)
        print('scene arrangement sampling')
        return self.diffusion.arrange_samples_ddim((batch_size, num_points, point_dim), device, condition=condition,
                                                   condition_cross=condition_cross, input_boxes=input_boxes,
                                                   sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta, **seeded,
                                                   **solver)

    @torch.no_grad()
    def complete_scene(self, room_mask, num_points, point_dim, partial_boxes, batch_size=1, ret_traj=False, ddim=False,
                       clip_denoised=False, batch_seeds=None, device="cpu", keep_empty=False, sampling_timesteps=None,
                       ddim_sampling_eta=0.0, scene_seeds=None, collision_scale=None, collision_steps=None, sampling_solver=None,
                       wall_scale=None, wall_steps=None, room_side=None, resample=None, resample_steps=None):
        """reference :335-340.  ``sampling_timesteps=S`` runs the strided loop (``complete_samples_ragged_ddim`` with uniform counts:
        every scene is given all rows of ``partial_boxes``) instead of the T-step one; the post-filter is the same (batch row 0).
        x_start is always clamped there and ``clip_denoised`` / ``ret_traj`` play no part.  ``collision_scale`` / ``collision_steps``:
        collision steering (see ``sample``); the given objects repel the free ones and are never moved.  ``sampling_solver``:
        "dpmpp_2m" with ``sampling_timesteps`` (see ``sample``).  ``resample`` / ``resample_steps``: RePaint's resampling jumps (see
        ``complete_scene_batched``); the T-step call is then that method's (``_complete_tstep`` with uniform counts), the post-filter this
        one's."""
        jumps = self._check_resample(resample, resample_steps, sampling_solver, ret_traj, "complete_scene")
        solver = self._check_solver(sampling_solver, sampling_timesteps, ddim_sampling_eta, "complete_scene")
        self._check_room(room_mask, batch_size, "complete_scene")
        if jumps and sampling_timesteps is None:                  # sample() does not take the keyword: the T-step call of complete_scene_batched
            shape = (batch_size, num_points, point_dim)
            steer = self._check_steering(collision_scale, collision_steps, wall_scale, wall_steps, room_side, room_mask,
                                         shape, what="complete_scene")
            seeded = self._seeded(scene_seeds, batch_seeds, batch_size, room_mask.device)
            padded, counts = self._ragged_partial(partial_boxes, None, batch_size, num_points, point_dim, room_mask.device)
            samples = self._complete_tstep(room_mask, num_points, point_dim, padded, counts, batch_size, clip_denoised, seeded, steer, jumps,
                                           "complete_scene")
            return self.delete_empty_from_network_samples(samples, device=device, keep_empty=keep_empty)
        if sampling_timesteps is not None:
            S, eta = self._check_strided(sampling_timesteps, ddim_sampling_eta)
            steer = self._check_steering(collision_scale, collision_steps, wall_scale, wall_steps, room_side, room_mask,
                                         (batch_size, num_points, point_dim), what="complete_scene")
            seeded = self._seeded(scene_seeds, batch_seeds, batch_size, room_mask.device)
            padded, counts = self._ragged_partial(partial_boxes, None, batch_size, num_points, point_dim, room_mask.device)
            samples = self._complete_strided(room_mask, num_points, point_dim, padded, counts, batch_size, S, eta, seeded, steer, solver,
                                             jumps)
            return self.delete_empty_from_network_samples(samples, device=device, keep_empty=keep_empty)
        samples = self.sample(room_mask, num_points, point_dim, batch_size, partial_boxes=partial_boxes,
                              ret_traj=ret_traj, ddim=ddim, clip_denoised=clip_denoised, batch_seeds=batch_seeds,
                              **_seed_kwargs(scene_seeds), **_steer_kwargs(collision_scale, collision_steps),
                              **_wall_kwargs(wall_scale, wall_steps, room_side))
        return self.delete_empty_from_network_samples(samples, device=device, keep_empty=keep_empty)

    @torch.no_grad()
    def arrange_scene(self, room_mask, num_points, point_dim, input_boxes, batch_size=1, ret_traj=False, ddim=False,
                      clip_denoised=False, batch_seeds=None, device="cpu", keep_empty=False, sampling_timesteps=None,
                      ddim_sampling_eta=0.0, scene_seeds=None, collision_scale=None, collision_steps=None, sampling_solver=None,
                      wall_scale=None, wall_steps=None, room_side=None):
        """reference :342-347.  ``sampling_timesteps=S`` runs ``arrange_samples_ddim`` (S strided steps) instead of the T-step loop.
        ``collision_scale`` / ``collision_steps`` are refused (ValueError): the loop diffuses [translation | angle] only.
        ``sampling_solver``: "dpmpp_2m" with ``sampling_timesteps`` (see ``sample``)."""
        self._check_steering(collision_scale, collision_steps, wall_scale, wall_steps, room_side, room_mask,
                             (batch_size, num_points, point_dim), input_boxes, what="arrange_scene")
        solver = self._check_solver(sampling_solver, sampling_timesteps, ddim_sampling_eta, "arrange_scene")
        self._check_room(room_mask, batch_size, "arrange_scene")
        if sampling_timesteps is not None:
            S, eta = self._check_strided(sampling_timesteps, ddim_sampling_eta)
            seeded = self._seeded(scene_seeds, batch_seeds, batch_size, room_mask.device)
            samples = self._arrange_strided(room_mask, num_points, point_dim, input_boxes, batch_size, S, eta, seeded, solver)
            return self.delete_empty_from_network_samples(samples, device=device, keep_empty=keep_empty)
        samples = self.sample(room_mask, num_points, point_dim, batch_size, input_boxes=input_boxes, ret_traj=ret_traj,
                              ddim=ddim, clip_denoised=clip_denoised, batch_seeds=batch_seeds, **_seed_kwargs(scene_seeds))
        return self.delete_empty_from_network_samples(samples, device=device, keep_empty=keep_empty)

    # ------------------------------------------------------------------------------------ post-filter
    def _keep_rows(self, empty_logit_row0, keep_empty):
        """Rows kept by the reference loop (:377-380, :424-427): drop slot i when the 'empty' logit of BATCH ROW 0
        is >= 0 (network samples) -- the decision is shared by the whole batch, as in the reference."""
        n = empty_logit_row0.shape[0]
        if keep_empty:
            return torch.arange(n)
        return torch.nonzero(~empty_logit_row0, as_tuple=False).flatten()

    def _split_boxes(self, rows):
        """(B, K, C) kept rows -> the reference's output dict (raw class scores, :383-386; CPU tensors, :390-406)."""
        tr, sz, bb, nc = self.translation_dim, self.size_dim, self.bbox_dim, self.class_dim
        out = {
            "class_labels": rows[:, :, bb:bb + nc - 1].contiguous(),
            "translations": rows[:, :, 0:tr].contiguous(),
            "sizes": rows[:, :, tr:tr + sz].contiguous(),
            "angles": rows[:, :, tr + sz:bb].contiguous(),
        }
        if self.objfeat_dim > 0:
            out["objfeats"] = rows[:, :, bb + nc:bb + nc + self.objfeat_dim].contiguous()
        return out

    @torch.no_grad()
    def delete_empty_from_network_samples(self, samples, device="cpu", keep_empty=False):
        """Reference :351-406.  Its loop takes the keep / drop decision of every slot from BATCH ROW 0 (:379) (and only runs
        for batch_size 1: its accumulators are (1, 0, .) tensors); here that decision is applied to the whole batch, so
        B = 1 is exactly the reference and B > 1 returns equally long scenes.  Samples on a HIP device are compacted there
        (dsc_postfilter_compact_f32, one launch) and cross to the host once; per-scene filtering of a batch is
        ``delete_empty_per_scene``."""
        samples = samples.detach()
        bb, nc = self.bbox_dim, self.class_dim
        if samples.is_cuda and samples.dtype == torch.float32 and samples.shape[1] <= 192:
            from .. import ops
            packed, counts = ops.postfilter_compact(samples.contiguous(), bb + nc - 1, per_scene=False, keep_empty=keep_empty)
            k = int(counts[0].item())
            return self._split_boxes(packed[:, :k].to("cpu"))
        samples = samples.to("cpu")
        keep = self._keep_rows(samples[0, :, bb + nc - 1] >= 0, keep_empty)
        return self._split_boxes(samples[:, keep])

    @torch.no_grad()
    def delete_empty_per_scene(self, samples, keep_empty=False):
        """Batched generation: every scene of ``samples`` (B, N, C) is filtered by ITS OWN 'empty' logits, i.e. the reference
        method applied to each scene alone.  One device launch + one device->host copy; returns a list of B dicts (the
        reference's keys, leading dimension 1)."""
        from .. import ops
        samples = samples.detach().contiguous()
        packed, counts = ops.postfilter_compact(samples, self.bbox_dim + self.class_dim - 1, per_scene=True,
                                                keep_empty=keep_empty)
        packed, counts = packed.to("cpu"), counts.to("cpu").tolist()
        return [self._split_boxes(packed[b:b + 1, :counts[b]]) for b in range(samples.shape[0])]

    @torch.no_grad()
    def generate_layout_batched(self, room_mask, num_points, point_dim, batch_size, text=None, clip_denoised=False,
                                batch_seeds=None, keep_empty=False, sampling_timesteps=None, ddim_sampling_eta=0.0,
                                guidance_scale=None, scene_seeds=None, collision_scale=None, collision_steps=None,
                                sampling_solver=None,
                                wall_scale=None, wall_steps=None, room_side=None):
        """``generate_layout`` for a whole batch: one reverse loop for ``batch_size`` scenes, each post-filtered on its own.
        ``guidance_scale``: a float or one classifier-free guidance scale per scene (see ``sample``).  ``scene_seeds``: one seed per
        scene (``_seeded``): scene b can then be regenerated alone, or the batch split over calls and devices.  ``collision_scale`` /
        ``collision_steps``: collision steering, a weight per scene (see ``sample``).  ``sampling_solver``: "dpmpp_2m" with
        ``sampling_timesteps`` (see ``sample``).  ``wall_scale`` / ``wall_steps`` / ``room_side``: floor-plan steering on ``room_mask``,
        a weight per scene (see ``sample``)."""
        samples = self.sample(room_mask, num_points, point_dim, batch_size, text=text, clip_denoised=clip_denoised,
                              batch_seeds=batch_seeds, **_ddim_kwargs(sampling_timesteps, ddim_sampling_eta),
                              **_guidance_kwargs(guidance_scale), **_seed_kwargs(scene_seeds),
                              **_steer_kwargs(collision_scale, collision_steps),
                              **_wall_kwargs(wall_scale, wall_steps, room_side), **_solver_kwargs(sampling_solver))
        return self.delete_empty_per_scene(samples, keep_empty=keep_empty)

    def _ragged_partial(self, partial_boxes, num_partial, batch_size, num_points, point_dim, device):
        """Normalise the given objects of ``complete_scene_batched``: a list of B (P_b, C) tensors, or a padded (B, Pmax, C) tensor
        with counts (``num_partial=None``: every scene is given all Pmax rows) -> ((B, num_points, C) float32 on ``device``, rows at or
        beyond a scene's count ZERO, and the counts as a list of B ints).  ValueError names the offending scene."""
        if isinstance(partial_boxes, (list, tuple)):
            if num_partial is not None:
                raise ValueError("num_partial goes with a padded (B, Pmax, C) tensor; a list of scenes carries its own counts")
            if len(partial_boxes) != batch_size:
                raise ValueError("partial_boxes lists %d scenes for a batch of %d" % (len(partial_boxes), batch_size))
            scenes = []
            for b, boxes in enumerate(partial_boxes):
                if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2:
                    raise ValueError("scene %d: partial boxes must be a (P, %d) tensor" % (b, point_dim))
                scenes.append(boxes)
            counts = [int(boxes.shape[0]) for boxes in scenes]
        else:
            if not isinstance(partial_boxes, torch.Tensor) or partial_boxes.dim() != 3:
                raise ValueError("partial_boxes must be a list of (P_b, %d) tensors or a padded (B, Pmax, %d) tensor"
                                 % (point_dim, point_dim))
            if partial_boxes.shape[0] != batch_size:
                raise ValueError("partial_boxes holds %d scenes for a batch of %d" % (partial_boxes.shape[0], batch_size))
            pmax = int(partial_boxes.shape[1])
            if num_partial is None:
                counts = [pmax] * batch_size
            else:
                counts = num_partial.tolist() if isinstance(num_partial, torch.Tensor) else list(num_partial)
                if len(counts) != batch_size:
                    raise ValueError("num_partial has %d entries for a batch of %d" % (len(counts), batch_size))
                for b, v in enumerate(counts):
                    if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= pmax:
                        raise ValueError("scene %d: num_partial %r outside [0, %d], the rows of partial_boxes" % (b, v, pmax))
                counts = [int(v) for v in counts]
            scenes = [partial_boxes[b, :counts[b]] for b in range(batch_size)]
        padded = torch.zeros((batch_size, num_points, point_dim), dtype=torch.float32, device=device)
        for b, boxes in enumerate(scenes):
            if boxes.shape[-1] != point_dim:
                raise ValueError("scene %d: partial boxes have %d channels, the model has %d" % (b, boxes.shape[-1], point_dim))
            if counts[b] > num_points:
                raise ValueError("scene %d: %d given objects, more than num_points = %d" % (b, counts[b], num_points))
            if counts[b]:
                padded[b, :counts[b]] = boxes.to(device=device, dtype=torch.float32)
        return padded, counts

    @torch.no_grad()
    def complete_scene_batched(self, room_mask, num_points, point_dim, partial_boxes, num_partial=None, batch_size=None,
                               clip_denoised=False, batch_seeds=None, keep_empty=False, sampling_timesteps=None,
                               ddim_sampling_eta=0.0, scene_seeds=None, collision_scale=None, collision_steps=None,
                               sampling_solver=None,
                               wall_scale=None, wall_steps=None, room_side=None, resample=None, resample_steps=None):
        """``complete_scene`` for a whole batch in which every scene is given ITS OWN number of objects: one reverse loop
        (``complete_samples_ragged``), each scene post-filtered on its own -- scene b is ``complete_scene`` at batch_size 1 with
        partial_boxes[b].  ``partial_boxes``: a list of B (P_b, C) tensors, or a padded (B, Pmax, C) tensor with ``num_partial`` (B,)
        (without it: all Pmax rows of every scene).  0 <= P_b <= num_points; 0 is plain generation.  The given rows are padded with
        zeros to ``num_points``, so one captured graph serves every mix of counts and a ``room_partial_condition`` model sees the
        reference's cat([partial, zeros]) of each scene.  Returns a list of B dicts; given rows are filtered like any other row.
        ``sampling_timesteps=S`` runs the strided loop (``complete_samples_ragged_ddim``: S DDIM steps at ``ddim_sampling_eta``, the
        given rows re-noised with fresh noise before every model call -- so at eta = 0 the free rows are deterministic given x_T and
        those draws, not given x_T alone; x_start always clamped, ``clip_denoised`` ignored) instead of the T-step one.
        ``collision_scale`` / ``collision_steps``: collision steering, a weight per scene (see ``sample``); the given objects repel the
        free ones and are never moved.  ``sampling_solver``: "dpmpp_2m" with ``sampling_timesteps`` (see ``sample``).
        ``resample=(jump_length, n_resample)`` (None: this method as it was, same code path, same draws): RePaint's resampling jumps
        -- after every stretch of ``jump_length`` reverse steps the whole state is diffused forward again by that many steps in one
        draw and the stretch is walked down once more, ``n_resample`` times in all, so the free part sees the given part several times
        at each noise level; ``resample_steps=K`` resamples only where the timestep is below K.  The cost is model
        calls: U + (n_resample - 1) * jump_length per jump point (GaussianDiffusion.resample_schedule).  Combines with
        ``sampling_timesteps``, steering and seeds; refused with ``sampling_solver`` and on room_partial_condition /
        room_arrange_condition models."""
        device = room_mask.device
        if batch_size is None:
            batch_size = len(partial_boxes) if isinstance(partial_boxes, (list, tuple)) else int(partial_boxes.shape[0])
        jumps = self._check_resample(resample, resample_steps, sampling_solver, False, "complete_scene_batched")
        solver = self._check_solver(sampling_solver, sampling_timesteps, ddim_sampling_eta, "complete_scene_batched")
        self._check_room(room_mask, batch_size, "complete_scene_batched")
        steer = self._check_steering(collision_scale, collision_steps, wall_scale, wall_steps, room_side, room_mask,
                                     (batch_size, num_points, point_dim), what="complete_scene_batched")
        seeded = self._seeded(scene_seeds, batch_seeds, batch_size, device)
        if sampling_timesteps is not None:
            S, eta = self._check_strided(sampling_timesteps, ddim_sampling_eta)
            padded, counts = self._ragged_partial(partial_boxes, num_partial, batch_size, num_points, point_dim, device)
            samples = self._complete_strided(room_mask, num_points, point_dim, padded, counts, batch_size, S, eta, seeded, steer, solver,
                                             jumps)
            return self.delete_empty_per_scene(samples, keep_empty=keep_empty)
        padded, counts = self._ragged_partial(partial_boxes, num_partial, batch_size, num_points, point_dim, device)
        samples = self._complete_tstep(room_mask, num_points, point_dim, padded, counts, batch_size, clip_denoised, seeded, steer, jumps)
        return self.delete_empty_per_scene(samples, keep_empty=keep_empty)

    def _complete_tstep(self, room_mask, num_points, point_dim, padded, counts, batch_size, clip_denoised, seeded={}, steer={}, resample={},
                        what="complete_scene_batched"):
        """The T-step completion call behind complete_scene_batched (and complete_scene under ``resample``): the condition assembly of
        ``sample`` (the CPU draw included), then ``complete_samples_ragged``."""
        device = room_mask.device
        noise = torch.randn((batch_size, num_points, point_dim))   # CPU draw kept, as in sample (:232)
        if self.room_arrange_condition:
            raise ValueError("%s: a room_arrange_condition model re-arranges scenes (arrange_scene_batched)" % what)
        condition, condition_cross = self._sampling_conditions(room_mask, num_points, device, padded_partial=padded, batch_size=batch_size)
        print('scene completion sampling')
        return self.diffusion.complete_samples_ragged(noise.shape, device, condition=condition, condition_cross=condition_cross,
                                                      clip_denoised=clip_denoised, partial_boxes=padded, num_partial=counts, **seeded,
                                                      **steer, **resample)

    @torch.no_grad()
    def arrange_scene_batched(self, room_mask, num_points, point_dim, input_boxes, batch_size=None, clip_denoised=False,
                              batch_seeds=None, keep_empty=False, sampling_timesteps=None, ddim_sampling_eta=0.0, scene_seeds=None,
                              collision_scale=None, collision_steps=None, sampling_solver=None,
                              wall_scale=None, wall_steps=None, room_side=None):
        """``arrange_scene`` for a whole batch: one ``arrange_samples`` loop for the B scenes of ``input_boxes`` (B, num_points, C),
        each post-filtered on its own.  ``sampling_timesteps=S`` runs ``arrange_samples_ddim`` (S strided steps) instead.
        ``collision_scale`` / ``collision_steps`` are refused (ValueError): the loop diffuses [translation | angle] only.
        ``sampling_solver``: "dpmpp_2m" with ``sampling_timesteps`` (see ``sample``)."""
        self._check_steering(collision_scale, collision_steps, wall_scale, wall_steps, room_side, room_mask,
                             (1, num_points, point_dim), input_boxes, what="arrange_scene_batched")
        solver = self._check_solver(sampling_solver, sampling_timesteps, ddim_sampling_eta, "arrange_scene_batched")
        if not isinstance(input_boxes, torch.Tensor) or input_boxes.dim() != 3:
            raise ValueError("input_boxes must be a (B, %d, %d) tensor" % (num_points, point_dim))
        if batch_size is None:
            batch_size = int(input_boxes.shape[0])
        if input_boxes.shape[0] != batch_size:
            raise ValueError("input_boxes holds %d scenes for a batch of %d" % (input_boxes.shape[0], batch_size))
        if input_boxes.shape[1] != num_points or input_boxes.shape[2] != point_dim:
            raise ValueError("input_boxes: every scene must be (%d, %d), got %s" % (num_points, point_dim, tuple(input_boxes.shape[1:])))
        self._check_room(room_mask, batch_size, "arrange_scene_batched")
        if sampling_timesteps is not None:
            S, eta = self._check_strided(sampling_timesteps, ddim_sampling_eta)
            seeded = self._seeded(scene_seeds, batch_seeds, batch_size, room_mask.device)
            samples = self._arrange_strided(room_mask, num_points, point_dim, input_boxes, batch_size, S, eta, seeded, solver)
            return self.delete_empty_per_scene(samples, keep_empty=keep_empty)
        samples = self.sample(room_mask, num_points, point_dim, batch_size, input_boxes=input_boxes, clip_denoised=clip_denoised,
                              batch_seeds=batch_seeds, **_seed_kwargs(scene_seeds))
        return self.delete_empty_per_scene(samples, keep_empty=keep_empty)

    # ------------------------------------------------------------------------------------ element-wise in-painting
    ATTRIBUTES = ("translations", "sizes", "angles", "class_labels", "objfeats")

    def _attribute_channels(self, name):
        """Channel range [lo, hi) of an attribute in a scene row, the slices of ``_split_boxes`` ('class_labels' with the 'empty' column)."""
        tr, sz, bb, nc = self.translation_dim, self.size_dim, self.bbox_dim, self.class_dim
        if name == "objfeats" and self.objfeat_dim <= 0:
            raise ValueError("attributes: 'objfeats' on a model without object features (objfeat_dim = 0)")
        spans = {"translations": (0, tr), "sizes": (tr, tr + sz), "angles": (tr + sz, bb), "class_labels": (bb, bb + nc),
                 "objfeats": (bb + nc, bb + nc + self.objfeat_dim)}
        if name not in spans:
            raise ValueError("attributes: %r is not one of %s" % (name, self.ATTRIBUTES))
        return spans[name]

    def attribute_mask(self, rows, attributes, batch_size, num_points):
        """The (B, N, C) bool mask (CPU) of ``inpaint_scene_batched`` that marks ``attributes`` -- a subset of ATTRIBUTES, mapped to the
        channel ranges ``_split_boxes`` slices -- of the objects ``rows`` as given.  ``rows``: one count per scene (an int for all
        scenes, a sequence or 1-d integer tensor of B counts: rows [0, count)), a sequence of B index lists, or a (B, N) bool tensor.
        Masks combine with ``|``.  ValueError names the scene or argument."""
        B, N, C = int(batch_size), int(num_points), int(self.config["point_dim"])
        if isinstance(attributes, str):
            attributes = (attributes,)
        chan = torch.zeros(C, dtype=torch.bool)
        for name in attributes:
            lo, hi = self._attribute_channels(name)
            if hi > C:
                raise ValueError("attributes: %r spans channels [%d, %d) of a %d-channel model" % (name, lo, hi, C))
            chan[lo:hi] = True
        sel = torch.zeros((B, N), dtype=torch.bool)
        if isinstance(rows, torch.Tensor) and rows.dtype == torch.bool:
            if tuple(rows.shape) != (B, N):
                raise ValueError("rows: a bool tensor must be (%d, %d), got %s" % (B, N, tuple(rows.shape)))
            sel = rows.to("cpu").clone()
        else:
            if isinstance(rows, torch.Tensor):
                if rows.dim() > 1 or rows.dtype.is_floating_point:
                    raise ValueError("rows: an integer tensor must hold one count per scene, got %s %s" % (tuple(rows.shape), rows.dtype))
                rows = rows.tolist()
            if isinstance(rows, int) and not isinstance(rows, bool):
                rows = [rows] * B
            if not isinstance(rows, (list, tuple)) or len(rows) != B:
                raise ValueError("rows: one count or index list per scene (%d scenes) or a (%d, %d) bool tensor" % (B, B, N))
            for b, r in enumerate(rows):
                if isinstance(r, torch.Tensor) and r.dim() == 1 and not r.dtype.is_floating_point and r.dtype != torch.bool:
                    r = r.tolist()
                if isinstance(r, (list, tuple)):
                    for i in r:
                        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < N:
                            raise ValueError("scene %d: row index %r outside [0, %d)" % (b, i, N))
                        sel[b, i] = True
                elif isinstance(r, int) and not isinstance(r, bool):
                    if not 0 <= r <= N:
                        raise ValueError("scene %d: row count %r outside [0, %d]" % (b, r, N))
                    sel[b, :r] = True
                else:
                    raise ValueError("scene %d: rows must be a count or a list of indices, got %r" % (b, r))
        return sel[:, :, None] & chan[None, None, :]

    @torch.no_grad()
    def inpaint_scene_batched(self, room_mask, num_points, point_dim, boxes, known_mask, batch_size=None, text=None,
                              clip_denoised=False, batch_seeds=None, keep_empty=False, sampling_timesteps=None, ddim_sampling_eta=0.0,
                              scene_seeds=None, guidance_scale=None, collision_scale=None, collision_steps=None, sampling_solver=None,
                              wall_scale=None, wall_steps=None, room_side=None, resample=None, resample_steps=None):
        """Attribute-level in-painting of a batch: every element of ``boxes`` marked in ``known_mask`` is held fixed, the rest of each
        scene is sampled around it -- one reverse loop (``inpaint_samples``; ``sampling_timesteps=S``: ``inpaint_samples_ddim``, x_start
        always clamped and ``clip_denoised`` ignored), each scene post-filtered on its own.  ``boxes``: (B, num_points, point_dim) in
        the network's encoding, or a list of B (n_b <= num_points, point_dim) tensors, padded with zeros -- padded rows are never
        known.  ``known_mask``: (B, N, C) or (B, N) bool / uint8, e.g. from ``attribute_mask``.  Works on the ordinary unconditional,
        instance- or text-conditioned model (``text`` as in ``sample``); ``room_partial_condition`` / ``room_arrange_condition`` models
        are refused, their condition tensors already encode a prefix / a sub-shape.  Returns a list of B dicts; given elements are
        filtered like any others (a row whose given 'empty' logit is >= 0 is dropped).
        ``guidance_scale`` (None: this method as it was, same code path, same draws): a float or B per-scene classifier-free guidance
        scales of a text-conditioned model, as in ``sample`` -- the fixed elements pull the sample away from the prompt, the scale pulls
        it back (``inpaint_samples_guided`` / ``inpaint_samples_guided_ddim``).  Needs ``text``; refused, before anything is drawn, on a
        model without ``text_condition`` and on a text encoder that does not give (B, L, text_embed_dim) features.
        ``collision_scale`` / ``collision_steps``: collision steering, a weight per scene (see ``sample``); a known element enters the
        boxes with its known value and is never moved.  ``sampling_solver``: "dpmpp_2m" with ``sampling_timesteps`` (see ``sample``).
        ``resample`` / ``resample_steps``: RePaint's resampling jumps (see ``complete_scene_batched``), with or without ``text`` /
        ``guidance_scale``."""
        from .. import ops
        jumps = self._check_resample(resample, resample_steps, sampling_solver, False, "inpaint_scene_batched")
        solver = self._check_solver(sampling_solver, sampling_timesteps, ddim_sampling_eta, "inpaint_scene_batched")
        if self.room_partial_condition or self.room_arrange_condition:
            raise ValueError("inpaint_scene_batched: a room_partial_condition / room_arrange_condition model conditions on a prefix / a "
                             "sub-shape of the scene (complete_scene_batched, arrange_scene_batched)")
        if guidance_scale is not None:
            self._check_guidance(text)
        device = room_mask.device
        if batch_size is None:
            batch_size = len(boxes) if isinstance(boxes, (list, tuple)) else int(boxes.shape[0])
        B, N, C = int(batch_size), int(num_points), int(point_dim)
        self._check_room(room_mask, B, "inpaint_scene_batched")
        scale = None if guidance_scale is None else ops.guidance_scales(guidance_scale, B, "cpu")   # checked on the host; the loop uploads it
        steer = self._check_steering(collision_scale, collision_steps, wall_scale, wall_steps, room_side, room_mask,
                                     (B, N, C), what="inpaint_scene_batched")
        seeded = self._seeded(scene_seeds, batch_seeds, B, device)
        if isinstance(boxes, (list, tuple)):
            if len(boxes) != B:
                raise ValueError("boxes lists %d scenes for a batch of %d" % (len(boxes), B))
            known = torch.zeros((B, N, C), dtype=torch.float32, device=device)
            valid = torch.zeros((B, N), dtype=torch.bool)
            for b, sc in enumerate(boxes):
                if not isinstance(sc, torch.Tensor) or sc.dim() != 2 or sc.shape[1] != C or sc.shape[0] > N:
                    raise ValueError("scene %d: boxes must be a (n <= %d, %d) tensor, got %s" % (b, N, C, tuple(getattr(sc, "shape", ()))))
                known[b, :sc.shape[0]] = sc.to(device=device, dtype=torch.float32)
                valid[b, :sc.shape[0]] = True
        else:
            if not isinstance(boxes, torch.Tensor) or tuple(boxes.shape) != (B, N, C):
                raise ValueError("boxes must be a (%d, %d, %d) tensor or a list of %d (n, %d) tensors, got %s"
                                 % (B, N, C, B, C, tuple(getattr(boxes, "shape", ()))))
            known = boxes.to(device=device, dtype=torch.float32).contiguous()
            valid = None
        try:
            mask = ops.known_mask(known_mask, (B, N, C), "cpu" if valid is not None else device)
        except ValueError as e:
            raise ValueError("known_mask: %s" % e) from None
        if valid is not None:
            mask = (mask * valid[:, :, None].to(torch.uint8)).to(device).contiguous()
        if sampling_timesteps is not None:
            S, eta = self._check_strided(sampling_timesteps, ddim_sampling_eta)
        if scale is not None:                                      # the last refusal of the keyword, still before any draw
            condition, condition_cross = self._sampling_conditions(room_mask, N, device, text=text, batch_size=B)
            if condition_cross is None or condition_cross.dim() != 3:
                raise ValueError("guidance_scale: the text encoder must give (B, L, text_embed_dim) features, got %s (the null "
                                 "condition is defined on the cross-attention features)"
                                 % (None if condition_cross is None else tuple(condition_cross.shape),))
        torch.randn((B, N, C))                                     # CPU draw kept, as in sample (:232)
        if scale is None:
            condition, condition_cross = self._sampling_conditions(room_mask, N, device, text=text, batch_size=B)
        print('scene in-painting sampling')
        if scale is not None:
            guided = dict(condition=condition, condition_cross=condition_cross, guidance_scale=scale, known=known, mask=mask, **seeded,
                          **steer, **jumps)
            if sampling_timesteps is not None:
                samples = self.diffusion.inpaint_samples_guided_ddim((B, N, C), device, sampling_timesteps=S, ddim_sampling_eta=eta,
                                                                     **guided, **solver)
            else:
                samples = self.diffusion.inpaint_samples_guided((B, N, C), device, clip_denoised=clip_denoised, **guided)
        elif sampling_timesteps is not None:
            samples = self.diffusion.inpaint_samples_ddim((B, N, C), device, condition=condition, condition_cross=condition_cross,
                                                          known=known, mask=mask, sampling_timesteps=S, ddim_sampling_eta=eta, **seeded,
                                                          **steer, **solver, **jumps)
        else:
            samples = self.diffusion.inpaint_samples((B, N, C), device, condition=condition, condition_cross=condition_cross,
                                                     clip_denoised=clip_denoised, known=known, mask=mask, **seeded, **steer, **jumps)
        return self.delete_empty_per_scene(samples, keep_empty=keep_empty)

    @torch.no_grad()
    def delete_empty_boxes(self, samples_dict, device="cpu", keep_empty=False):
        cl = samples_dict["class_labels"].detach().to("cpu")
        keep = self._keep_rows(cl[0, :, -1] > 0, keep_empty)
        out = {"class_labels": cl[:, keep, :self.class_dim - 1].contiguous()}
        for k in ("translations", "sizes", "angles") + (("objfeats",) if self.objfeat_dim > 0 else ()):
            out[k] = samples_dict[k].detach().to("cpu")[:, keep, :].contiguous()
        return out


def _ddim_kwargs(sampling_timesteps, ddim_sampling_eta):
    """The DDIM keywords ``sample`` receives: none at all on the DDPM path, so that call stays what it was."""
    if sampling_timesteps is None:
        return {}
    return dict(sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta)


def _seed_kwargs(scene_seeds):
    """The seed keyword ``sample`` receives: none at all without seeds, so that call stays what it was."""
    return {} if scene_seeds is None else dict(scene_seeds=scene_seeds)


def _steer_kwargs(collision_scale, collision_steps):
    """The steering keywords ``sample`` receives: none at all without steering, so that call stays what it was."""
    if collision_scale is None and collision_steps is None:
        return {}
    return dict(collision_scale=collision_scale, collision_steps=collision_steps)


def _wall_kwargs(wall_scale, wall_steps, room_side):
    """The floor-plan keywords ``sample`` receives: none at all without them, so that call stays what it was."""
    if wall_scale is None and wall_steps is None and room_side is None:
        return {}
    return dict(wall_scale=wall_scale, wall_steps=wall_steps, room_side=room_side)


def _solver_kwargs(sampling_solver):
    """The solver keyword ``sample`` receives: none at all without a solver, so that call stays what it was."""
    return {} if sampling_solver is None else dict(sampling_solver=sampling_solver)


def _guidance_kwargs(guidance_scale):
    """The guidance keyword ``sample`` receives: none at all without guidance, so that call stays what it was."""
    return {} if guidance_scale is None else dict(guidance_scale=guidance_scale)


def train_on_batch(model, optimizer, sample_params, config):
    """reference :456-473: zero_grad, loss, backward, clip_grad_norm_(max_grad_norm), optimizer step.

    Default path: the static training plan (train_step.py / train_plan.py) -- forward, loss and backward are one hipGraph
    replay that leaves every gradient in the flat buffer G; under torch.distributed the buckets of G are all-reduced over
    RCCL while the backward is still running, so every rank clips and steps identically.  Configurations the plan does not
    cover run the same HIP kernels under torch.autograd (autograd_ops.py).  All logged scalars are fetched with one
    device->host copy."""
    from ..ddp import average_gradients, clip_grad_norm_fused, overlapped_reducer
    from ..train_step import loss_step, plan_supported
    if plan_supported(model):
        # optimizer.zero_grad(): every gradient is OVERWRITTEN by the plan, so nothing is zeroed or freed; only a pending
        # deferred clip coefficient is cancelled (FusedAdam)
        if hasattr(optimizer, "cancel_pending_clip"):
            optimizer.cancel_pending_clip()
        loss, loss_dict, _ = loss_step(model, sample_params, backward=True)
    else:
        optimizer.zero_grad()
        reducer = overlapped_reducer(model)      # None on one GPU; hooks launch bucket all-reduces during backward
        loss, loss_dict = model.get_loss(sample_params)
        loss.backward()
        if reducer is not None:
            reducer.finish()
        else:
            average_gradients(model)             # no-op on one GPU; DSC_DDP_OVERLAP=0 selects this post-backward form
    if hasattr(optimizer, "clip_grad_norm_"):         # FusedAdam: norm + coefficient on the device, applied in step()
        grad_norm = optimizer.clip_grad_norm_(config["training"]["max_grad_norm"])
    else:
        grad_norm = clip_grad_norm_fused(model.parameters(), config["training"]["max_grad_norm"])
    keys = list(loss_dict.keys())
    packed_t = torch.stack([loss.detach(), grad_norm.detach()] + [loss_dict[k].detach() for k in keys])
    lr = optimizer.param_groups[0]['lr']
    if packed_t.is_cuda:
        # The logged scalars cross to the host ASYNCHRONOUSLY (pinned buffer + event) and the optimizer step is enqueued before the
        # host waits for them: the device runs the Adam sweep while the copy lands and the host gets on with the next batch.  (The
        # reference reads 11 .item() values, then steps: the values are the same -- everything logged is computed before the step --
        # but a blocking read in front of step() left the GPU idle for ~0.25 ms per step, profiles/r03_train_kernel_trace.txt.)
        host = getattr(model, "_dsc_scalars_host", None)
        if host is None or host.numel() != packed_t.numel():
            host = torch.empty(packed_t.numel(), dtype=torch.float32).pin_memory()
            object.__setattr__(model, "_dsc_scalars_host", host)
        host.copy_(packed_t, non_blocking=True)
        landed = torch.cuda.Event()
        landed.record(torch.cuda.current_stream(packed_t.device))
        optimizer.step()
        landed.synchronize()
        packed = host.tolist()
    else:
        packed = packed_t.tolist()
        optimizer.step()
    logger = StatsLogger.instance()
    for k, v in zip(keys, packed[2:]):
        logger[k].value = v
    logger["gradnorm"].value = packed[1]
    logger["lr"].value = lr
    from .._lib import check_indices
    check_indices("train_on_batch")            # DSC_CHECK_INDICES=1: a clamped (out-of-range) device timestep is an error, as in the reference
    return packed[0]


@torch.no_grad()
def validate_on_batch(model, sample_params, config):
    from ..train_step import loss_step, plan_supported
    if plan_supported(model):
        loss, loss_dict, _ = loss_step(model, sample_params, backward=False)
    else:
        loss, loss_dict = model.get_loss(sample_params)
    keys = list(loss_dict.keys())
    packed = torch.stack([loss.detach()] + [loss_dict[k].detach() for k in keys]).tolist()
    for k, v in zip(keys, packed[1:]):
        StatsLogger.instance()[k].value = v
    return packed[0]
