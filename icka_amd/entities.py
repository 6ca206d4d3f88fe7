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
from .crf import CRF, CrfPosterior, DeviceTags, NBestPaths


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

    def nbest(self, emissions: torch.Tensor, mask: Optional[torch.Tensor] = None, nbest: int = 1) -> "NBestEntities":
        """The entities of the ``nbest`` best paths of every sample: one ``CRF.decode_nbest`` launch, then one posterior launch
        per rank; no host sync until ``NBestEntities.tolist()``.  A sample with fewer than ``nbest`` distinct paths has -1 tags
        at the ranks it lacks; the posterior kernel is given the sample's rank-0 path there instead (so that it refuses
        nothing) and ``tolist()`` leaves those ranks out."""
        paths = self.crf.decode_nbest(emissions, mask, nbest)
        table = self.table(emissions.device)
        first = paths.rank(0)
        posts = []
        for r in range(nbest):
            tags = first
            if r > 0:
                row = paths.tags[r]
                tags = DeviceTags(paths.lens, torch.where(row < 0, first.tags_flat, row))
            posts.append(self.crf.posterior(emissions, tags, mask, label_table=table))
        return NBestEntities(paths, posts, self.types)


class NBestEntities(object):
    """What ``EntityDecoder.nbest`` returns: ``paths`` (the ``NBestPaths``), ``posteriors`` (one ``CrfPosterior`` per rank:
    ``posteriors[r].seq_logp`` is the log-probability of rank r) and ``types`` (type names by type id)."""

    def __init__(self, paths: NBestPaths, posteriors: Sequence[CrfPosterior], types: Sequence[str]):
        self.paths = paths
        self.posteriors = list(posteriors)
        self.types = list(types)

    def tolist(self) -> List[List[Tuple[str, int, int, float, Tuple[int, ...]]]]:
        """Per sample the union over its ranks of the entities, as ``(type_name, start, end, confidence, ranks)``: end
        exclusive, ``confidence`` the exact posterior of the tag span (as in ``Entities``; it does not depend on the rest of
        the path, and the value of the lowest rank that holds the span is reported), ``ranks`` the ascending tuple of the
        ranks whose path holds the entity.  Where ranks spell one entity with different tags (``B-PER I-PER`` and
        ``I-PER I-PER`` at the start of a path), ``confidence`` is the sum of the posteriors of these spans: the events
        exclude each other, so it is the probability that the positions carry one of the spellings seen.  Sorted by descending confidence, then ``(start, end, type_name)``.  The only call
        that syncs the host: every buffer goes over in one copy, the union and the sort run on the host.  Raises ValueError
        when the posterior kernel refused a sample."""
        parts = [self.paths.joint] + [p.joint for p in self.posteriors]
        h = torch.cat(parts).cpu()
        hp, o = self.paths.unpack(h[:parts[0].numel()]), parts[0].numel()
        ranks = []
        for p in self.posteriors:
            ranks.append(p.unpack(h[o:o + p.joint.numel()]))
            o += p.joint.numel()
        bad = sum(hr["bad"] for hr in ranks)
        if bad != 0:
            raise ValueError("EntityDecoder.nbest: the posterior kernel refused %d path(s)" % bad)
        out, off = [], 0
        for b, n in enumerate(hp["lens"]):
            found = {}      # (type id, start, end) -> [{span tags: confidence}, ranks]
            for r in range(hp["n_paths"][b]):
                hr = ranks[r]
                for k in range(off, off + hr["n_ent"][b]):
                    ty, s, e = hr["ent"][3 * k:3 * k + 3]
                    confs, rs = found.setdefault((ty, s, e), [{}, []])
                    confs.setdefault(tuple(hp["tags"][r][off + s:off + e]), hr["ent_conf"][k])
                    rs.append(r)
            rows = [(self.types[ty], s, e, sum(confs.values()), tuple(rs)) for (ty, s, e), (confs, rs) in found.items()]
            rows.sort(key=lambda x: (-x[3], x[1], x[2], x[0]))
            out.append(rows)
            off += n
        return out
