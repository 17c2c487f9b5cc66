"""MAE pretraining task module.

Parity: ``PretrainModule`` (/root/reference/src/pretraining.py:76-122) and the MAE branch of
``ViT.__call__`` (/root/reference/src/modeling.py:245-267).  Owns ``image_mask_embedding``
(1,1,d), ``decoder_proj`` (D->d) and ``decoder_image_output`` (d->p*p*3).

Differences by design (documented in SURVEY.md §2.9):
* Q2 fixed: the number of mask tokens is ``N - keep`` (the reference uses ``int(N*ratio)``,
  which silently clamps a gather when ``int(N*ratio) + int(N*(1-ratio)) != N``).
* mask-first embedding (see models/vit.py docstring); the final encoder LayerNorm feeds the
  decoder projection directly in the compute dtype.
* the decoder's final LayerNorm and the prediction GEMM only run on the 196 patch rows (the
  reference computes them for the 3 CLS rows too and then discards those rows).
"""

from __future__ import annotations

import torch

from ..config import DecoderConfig, ViTConfig
from ..data.constants import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD
from ..ops import attn_maps as AM
from ..ops import attn_stats as AS
from ..ops import mae as mae_ops
from ..utils.mae import masking_ids
from .params import ParamStore, trunc_normal_
from .vit import Dense, JumboViT, MAEDecoder, cls_features


class PretrainModel:
    def __init__(self, vit_cfg: ViTConfig, dec_cfg: DecoderConfig, norm_pix_loss: bool = False,
                 mask_mode: str = "shared"):
        assert vit_cfg.image_mask_ratio is not None
        self.cfg, self.dec_cfg = vit_cfg, dec_cfg
        self.norm_pix_loss = norm_pix_loss
        self.mask_mode = mask_mode
        self.store = ParamStore()
        s = self.store
        self.encoder = JumboViT(s, vit_cfg, ("model",))
        d = dec_cfg.dec_dim
        self.mask_token = s.handle(s.add(("image_mask_embedding",), (1, 1, d), trunc_normal_))
        self.decoder_proj = Dense(s, ("decoder_proj",), vit_cfg.dim, d)
        s.pad()
        self.decoder = MAEDecoder(s, dec_cfg, ("decoder_model",))
        self.decoder_image_output = Dense(s, ("decoder_image_output",), d, vit_cfg.patch_size ** 2 * 3)
        s.pad()

    # ------------------------------------------------------------------------ setup
    def to(self, device, compute_dtype=torch.float32, seed: int = 0):
        g = torch.Generator(device=device).manual_seed(seed)
        self.store.finalize(device, compute_dtype, g)
        return self

    @property
    def device(self):
        return self.store.master.device

    # ------------------------------------------------------------------------ forward
    def normalize(self, images_u8: torch.Tensor) -> torch.Tensor:
        """uint8 NCHW -> normalized float32 patches [B, N, p*p*3] (pretraining.py:90-91,113)."""
        return mae_ops.normalized_patches(images_u8, self.cfg.patch_size)

    def draw_mask(self, batch: int, noise_rng: torch.Generator | None, noise: torch.Tensor | None = None):
        n = self.cfg.seq_patches
        if noise is None:
            shape = (n,) if self.mask_mode == "shared" else (batch, n)
            noise = torch.rand(shape, generator=noise_rng, device=self.device)
        return masking_ids(noise, self.cfg.keep_len)

    def _predict(self, images_u8: torch.Tensor, rngs: dict, det: bool, enc_det: bool,
                 noise: torch.Tensor | None):
        """Mask, encode the kept patches, decode every patch: (pred [B, N, p*p*3], mask,
        (ids_shuffle, ids_restore, ids_keep))."""
        cfg = self.cfg
        B = images_u8.shape[0]
        C = cfg.num_cls_tokens
        N, K = cfg.seq_patches, cfg.keep_len
        ids_shuffle, ids_restore, ids_keep, mask = self.draw_mask(B, rngs.get("noise"), noise)
        # mask-first: only the kept patches are read (uint8 -> normalized bf16 GEMM rows)
        rows = mae_ops.kept_patches(images_u8, ids_keep, cfg.patch_size, self.store.compute_dtype)
        drop = rngs.get("dropout")
        x = self.encoder.embed_rows(rows, ids_keep, B)
        x = self.encoder.blocks(x, drop, det=enc_det, ids=ids_keep)
        h = self.encoder.norm(x)  # [B*(C+K), D]
        y = self.decoder_proj(h).view(B, C + K, -1)
        dec_in = mae_ops.unshuffle_fused(y, self.mask_token, ids_restore, self.decoder.posemb_table(y.device), C)
        xd = self.decoder.blocks(dec_in, drop, det=det)
        hd = self.decoder.dec_norm(xd, row0=C)  # [B*N, d] only patch rows are predicted
        pred = self.decoder_image_output(hd)  # [B*N, p*p*3]
        return pred.view(B, N, -1), mask, (ids_shuffle, ids_restore, ids_keep)

    def forward(self, images_u8: torch.Tensor, rngs: dict | None = None, det: bool = False,
                noise: torch.Tensor | None = None, per_sample: bool = False) -> dict:
        # encoder always runs with det=False (pretraining.py:92, quirk Q3)
        pred, mask, _ = self._predict(images_u8, rngs or {}, det, False, noise)
        # target pixels come straight from the uint8 images (no fp32 patch tensor)
        per_patch = mae_ops.patch_mse(pred, images_u8, self.cfg.patch_size, self.norm_pix_loss)
        loss = mae_ops.masked_mean_loss(per_patch, mask, per_sample)
        return {"loss": loss}

    __call__ = forward

    @torch.no_grad()
    def reconstruct(self, images_u8: torch.Tensor, noise: torch.Tensor | None = None, rngs: dict | None = None,
                    det: bool = True, fill: int = 127) -> dict:
        """Reconstruction images and their pixel-space quality.

        Returns ``recon`` / ``paste`` / ``masked`` (uint8 [B, 3, H, W], ops/mae.py
        ``reconstruct_panels``), ``mask`` [B, N] (1 = masked), ``err`` [B, N] and ``psnr_masked``
        [B] = -10 log10 of the mean of ``err`` over each image's masked patches ([0, 1] pixel scale,
        clamped and unrounded), comparable between --norm-pix-loss on and off.  Encoder and decoder
        both run with ``det`` (default True: a picture should not depend on a droppath draw).  No
        stream of the training ``rngs`` is touched unless the caller passes it; without ``noise``
        and without ``rngs["noise"]`` the mask comes from torch's default generator."""
        B = images_u8.shape[0]
        pred, mask, _ = self._predict(images_u8, rngs or {}, det, det, noise)
        out = mae_ops.reconstruct_panels(pred, images_u8, mask, self.cfg.patch_size, self.norm_pix_loss, fill)
        mask = (mask if mask.dim() == 2 else mask.unsqueeze(0).expand(B, mask.shape[0])).contiguous()
        mse = (out["err"] * mask).sum(-1) / mask.sum(-1)
        out["mask"] = mask
        out["psnr_masked"] = -10.0 * torch.log10(mse)
        return out

    @torch.no_grad()
    def features(self, images_u8: torch.Tensor) -> torch.Tensor:
        """[B, 3 * dim] fp32 encoder features as the classifier sees them: every patch (no masking),
        ``det=True``, the final LayerNorm on the three CLS rows (``FinetuneModel.features`` on the
        same parameters, bit for bit: both call ``cls_features``).  Touches no random stream."""
        rows = mae_ops.mixed_patches(images_u8, None, self.cfg.patch_size, self.store.compute_dtype)
        return cls_features(self.encoder, rows, images_u8.shape[0], None, True)

    @torch.no_grad()
    def attention_stats(self, images_u8: torch.Tensor, noise: torch.Tensor | None = None) -> dict:
        """``{name: float64 [H, 6]}`` (ops/attn_stats.py) of every attention layer in one masked
        ``det=True`` forward: ``layer_<i>`` for the encoder (on the kept patches), ``decoder/dec_layer_<i>``
        for the decoder -- the group names of ``optim/monitor.py group_name``.  ``noise`` as in
        ``reconstruct``; touches no stream of the training ``rngs``."""
        names = [f"layer_{i}" for i in range(len(self.encoder.layers))] + \
                [f"decoder/dec_layer_{i}" for i in range(len(self.decoder.layers))]
        return AS.collect_layers(names, lambda: self._predict(images_u8, {}, True, True, noise),
                                 self.cfg.num_cls_tokens)

    @torch.no_grad()
    def attention_maps(self, images_u8: torch.Tensor, alpha: float = 0.5, mode: str = "rollout") -> dict:
        """``{"maps": fp32 [B, n_cls, gh, gw], "cls_mass": fp32 [B, n_cls]}`` (ops/attn_maps.py): the CLS
        attention rollout (``mode="last"``: the last layer's head-mean CLS attention) over the encoder, from
        the forward ``features`` runs: every patch (no masking), ``det=True``.  The decoder does not run and
        no random stream is touched."""
        got = AM.collect_layers(lambda: self.features(images_u8), len(self.encoder.layers))
        g = self.cfg.grid
        return AM.maps_and_mass(got, got.heads, self.cfg.num_cls_tokens, g, g, alpha, mode)

    @torch.no_grad()
    def evaluate(self, images_u8: torch.Tensor, valid: torch.Tensor | None = None, rngs: dict | None = None) -> dict:
        """validation_step (pretraining.py:162-167): random masking and droppath stay active
        (det=False, quirk Q3); returns sums over valid images (fix for Q7: true mean later)."""
        per = self.forward(images_u8, rngs, det=False, per_sample=True)["loss"]
        v = torch.ones_like(per) if valid is None else valid.float()
        return {"loss": (per * v).sum(), "num_samples": v.sum()}

    # ------------------------------------------------------------------------ params
    def flax_params(self) -> dict:
        return self.store.to_flax_tree()

    def load_flax_params(self, tree: dict, strict: bool = True):
        return self.store.load_flax_tree(tree, strict=strict)


IMAGENET_MEAN = IMAGENET_DEFAULT_MEAN
IMAGENET_STD = IMAGENET_DEFAULT_STD
