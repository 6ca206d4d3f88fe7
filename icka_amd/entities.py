"""Entities of a tagged batch with their confidences, on the device.

``EntityDecoder`` turns emissions into the chunks of the Viterbi paths -- the rules of ``metrics.chunks``, i.e. the reference's
``ner_evaluate.get_chunks`` -- and gives every chunk the exact posterior probability of its tag span under the CRF
(``icka_crf_posterior``, csrc/crf_posterior.hip; the definitions are written out in include/icka_hip.h): two launches per batch
(``icka_crf_score_decode``, then the posterior kernel), no host sync until ``Entities.tolist()``.

    decoder = EntityDecoder.for_label_list(model.crf, label_list)
    em = model(..., mode=None)                      # emissions
    ents = decoder(em, mask=output_mask)            # capturable under torch.cuda.graph
    for sample in ents.tolist():                    # the one device-to-host copy
        for type_name, start, end, confidence in sample: ...

There is no gold label at inference time, so nothing is filtered by a skip list: ``start`` / ``end`` index the path (one tag per
position 0 and per position with ``mask != 0``)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import metrics
from .crf import CRF, CrfPosterior


class Entities(object):
    """What ``EntityDecoder`` returns: ``tags`` (the paths, a ``DeviceTags``), ``seq_logp`` (f32 [B]: log-probability of each
    path), ``log_z``, ``token_conf``, ``ent`` / ``ent_conf`` / ``n_ent`` / ``bad`` (the device buffers of ``CrfPosterior``, which
    is kept as ``posterior``) and ``types`` (type names by type id)."""

    def __init__(self, posterior: CrfPosterior, types: Sequence[str]):
        self.posterior = posterior
        self.types = list(types)
        self.tags, self.seq_logp, self.log_z, self.token_conf = posterior.tags, posterior.seq_logp, posterior.log_z, posterior.token_conf
        self.ent, self.ent_conf, self.n_ent, self.bad = posterior.ent, posterior.ent_conf, posterior.n_ent, posterior.bad

    def tolist(self) -> List[List[Tuple[str, int, int, float]]]:
        """Per sample the list of ``(type_name, start, end, confidence)``, end exclusive.  The only call that syncs the host (one
        copy).  Raises ValueError when the kernel refused a sample (a path that does not fit its mask, a tag id out of
        range)."""
        h = self.posterior.host()
        if h["bad"] != 0:
            raise ValueError("EntityDecoder: %d sample(s) were refused: a path whose length differs from its sample's number of "
                             "on-positions, or a tag id outside the CRF's range" % h["bad"])
        out, off = [], 0
        for b, n in enumerate(h["lens"]):
            rows = []
            for k in range(off, off + h["n_ent"][b]):
                ty, s, e = h["ent"][3 * k:3 * k + 3]
                rows.append((self.types[ty], s, e, h["ent_conf"][k]))
            out.append(rows)
            off += n
        return out


class EntityDecoder(object):
    """``decoder(emissions, mask=None, paths=None) -> Entities`` for a CRF and its label map (``{id: name}`` or the names by id;
    ``for_label_list`` takes the reference's label list, whose id 0 is "PAD")."""

    def __init__(self, crf: CRF, id_to_label, default: str = "O"):
        self.crf = crf
        self.names = metrics.label_names(id_to_label)
        self.default = default
        self.table_words, self.types = metrics.label_table(self.names, default, skip=())
        if len(self.names) < crf.num_tags:
            raise ValueError("the label map names %d ids, the CRF has %d tags" % (len(self.names), crf.num_tags))
        self._table: Optional[torch.Tensor] = None

    @classmethod
    def for_label_list(cls, crf: CRF, label_list: Sequence[str], **kw) -> "EntityDecoder":
        return cls(crf, metrics.label_list_map(label_list), **kw)

    def table(self, device) -> torch.Tensor:
        """The label table on ``device`` (uploaded once: call the decoder, or this, before capturing it in a graph)."""
        if self._table is None or self._table.device != torch.device(device):
            self._table = torch.tensor(self.table_words, dtype=torch.int32).to(device)
        return self._table

    def __call__(self, emissions: torch.Tensor, mask: Optional[torch.Tensor] = None, paths=None) -> Entities:
        post = self.crf.posterior(emissions, paths, mask, label_table=self.table(emissions.device))
        return Entities(post, self.types)
